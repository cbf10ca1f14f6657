"""Shared test helpers: device buffers for the C ABI, oracle model <-> device state."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from oracle import cql_oracle as O
from replay_cql_amd import _native as N

DEV = "cuda:0"
_KEEP = []   # device tensors handed to the C ABI as raw pointers must outlive the (asynchronous) call


def keep(t):
    _KEEP.append(t)
    return t


def release_kept():
    _KEEP.clear()


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    if dtype is not None:
        t = t.to(dtype)
    return keep(t.to(DEV).contiguous())


def bf16_dev(x_f32: np.ndarray) -> torch.Tensor:
    """fp32 numpy (any values) -> device bf16 tensor holding oracle-rounded values."""
    bits = O.bf16_bits(np.asarray(x_f32, dtype=np.float32)).astype(np.int16)
    return keep(torch.as_tensor(bits).to(DEV).view(torch.bfloat16).contiguous())


def bf16_to_np(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.float32).cpu().numpy()


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def sync():
    torch.cuda.synchronize()


def ws_bytes_tensor(nbytes: int) -> torch.Tensor:
    return torch.empty(int(nbytes), dtype=torch.uint8, device=DEV)


def small_log(U=64, N=257, seed=1, mean_len=12, max_len=40):
    u, i, t, r = O.synth_log(U, N, seed=seed, mean_len=mean_len, max_len=max_len)
    return O.build_csr(u, i, t, r, U)


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ---- shared case builders of the Q-head / top-K kernel tests (small shapes: test_gpu_kernels; published shapes:
# test_gpu_fullsize) ----------------------------------------------------------------------------------------------
def qhead_inputs(rows, Nn, d, dyadic, seed):
    rng = np.random.default_rng(seed)
    if dyadic:
        H = (rng.integers(-8, 9, (rows, d)) / 8.0).astype(np.float32)
        E = (rng.integers(-8, 9, (Nn, d)) / 8.0).astype(np.float32)
        b = (rng.integers(-16, 17, Nn) / 8.0).astype(np.float32)
    else:
        H = rng.standard_normal((rows, d)).astype(np.float32)
        E = (rng.standard_normal((Nn, d)) / np.sqrt(d)).astype(np.float32)
        b = (rng.standard_normal(Nn) * 0.3).astype(np.float32)
    return O.bf16_round(H), O.bf16_round(E), b


# ---- row-wise check of the softmax part of the Q-head gradients ------------------------------------------------------
# K of the row check.  tests/test_qhead_grad_rows_cpu.py is what justifies it (GPU-like roundings accepted, every listed
# fault rejected): change it there or nowhere.
ROWS_K = 4.0
ROWS_TINY = 1e-30             # absolute floor: rows whose every probability underflows fp32
_U32 = 2.0 ** -24             # fp32 unit roundoff
_BF16_SD = 2.0 ** -9          # standard deviation of the relative bf16 (RNE) rounding error of one P element
_T_SHIFT = 2.0 ** 40          # P is scaled by this before squaring in fp32: P^2 of P down to 1e-31 stays normal


class SoftmaxGradRef:
    """Dense softmax term of the Q-head gradients in float64 and its rounding-noise scale, UNSCALED (times `scale` gives
    the gradient).  Built by softmax_grad_reference; a test that checks several outputs of the same operands reuses it."""

    def __init__(self, scale, n_states, n_items):
        self.scale, self.n_states, self.n_items = float(scale), n_states, n_items
        self.dE = self.tE = self.cE = self.db = self.tb = self.dH = self.tH = self.cH = None
        self.arg = 0.0


def softmax_grad_reference(hb, lse, E_b, b_out, scale, items=True, states=True, chunk=None) -> SoftmaxGradRef:
    """P = exp(hb E_b^T + b_out - lse) in float64 from the kernels' own bf16 operands and the kernels' own lse, one item
    chunk at a time (B x chunk float64 score block: 64 MB), and per output element
        dense        dE[j] = sum_b P[b,j] hb[b],   db[j] = sum_b P[b,j],   dH[b] = sum_j P[b,j] E_b[j]
        t            sum of the squared terms (P x)^2, times 2^80         } float32: they only set
        c            sum of (bf16(P) - P) x, P rounded at the true scale  } the tolerance
    See softmax_grad_rows for how t becomes the noise scale."""
    H = np.asarray(hb, dtype=np.float32).astype(np.float64)
    E = np.asarray(E_b, dtype=np.float32)
    bo = np.asarray(b_out, dtype=np.float64)
    ls = np.asarray(lse, dtype=np.float64)
    B, d = H.shape
    Nn = E.shape[0]
    ref = SoftmaxGradRef(scale, B, Nn)
    if chunk is None:
        chunk = max(256, (1 << 23) // B // 256 * 256)
    H2 = (H * H).astype(np.float32)
    H32 = H.astype(np.float32)
    if items:
        ref.dE, ref.tE, ref.cE = np.zeros((Nn, d)), np.zeros((Nn, d), np.float32), np.zeros((Nn, d), np.float32)
        ref.db, ref.tb = np.zeros(Nn), np.zeros(Nn)
    if states:
        ref.dH, ref.tH, ref.cH = np.zeros((B, d)), np.zeros((B, d), np.float32), np.zeros((B, d), np.float32)
    amax = 0.0
    for lo in range(0, Nn, chunk):
        hi = min(Nn, lo + chunk)
        Ec = E[lo:hi].astype(np.float64)
        Z = H @ Ec.T
        Z += bo[lo:hi]
        amax = max(amax, float(np.abs(Z).max()))
        Z -= ls[:, None]
        P = np.exp(Z, out=Z)
        Ps = P * _T_SHIFT
        P2 = (Ps * Ps).astype(np.float32)
        P32 = P.astype(np.float32)
        u = P32.view(np.uint32)
        Cd = ((u + np.uint32(0x7FFF) + ((u >> 16) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32) - P32
        if items:
            ref.dE[lo:hi] = P.T @ H
            ref.tE[lo:hi] = P2.T @ H2
            ref.cE[lo:hi] = Cd.T @ H32
            ref.db[lo:hi] = P.sum(0)
            ref.tb[lo:hi] = P2.sum(0, dtype=np.float64)
        if states:
            ref.dH += P @ Ec
            ref.tH += P2 @ (Ec * Ec).astype(np.float32)
            ref.cH += Cd @ E[lo:hi]
        del Z, P, Ps, P2, P32, Cd
    ref.arg = amax + float(np.abs(ls).max())
    return ref


def _fp32_coef(n_terms, arg):
    # relative fp32 error of a sum of n_terms softmax terms (see softmax_grad_rows): accumulation + exponent argument
    return _U32 * (np.sqrt(n_terms) + 2.0 * arg + 4.0)


def _row_verdict(name, err, sig, K, group_sizes, out, offset=0):
    """err, sig: [rows, width] (or [rows]) of rows offset, offset + 1, ...  Keeps the worst ratio in out[name]; returns
    the failure line (empty list: every row passes)."""
    err = err.reshape(err.shape[0], -1)
    sig = sig.reshape(sig.shape[0], -1)
    en = np.sqrt(np.einsum("ij,ij->i", err, err))
    sn = np.sqrt(np.einsum("ij,ij->i", sig, sig))
    ratio = en / (sn + ROWS_TINY / K)
    out[name] = max(out.get(name, 0.0), float(ratio.max(initial=0.0)))
    bad = np.nonzero(en > K * sn + ROWS_TINY)[0]
    if bad.size == 0:
        return []
    worst = bad[np.argsort(-ratio[bad])][:6]
    rows = ", ".join(f"{offset + int(r)} (" + " ".join(f"/{g}:{(offset + int(r)) // g}" for g in group_sizes) +
                     f" err/sigma {ratio[r]:.3g})" for r in worst)
    return [f"{name}: {bad.size} of {err.shape[0]} rows over K = {K} sigma; worst: {rows}"]


def softmax_grad_rows(hb, lse, E_b, b_out, scale, g_E_out=None, g_b_out=None, dH=None, coef=None, act=None,
                      ref=None, K=ROWS_K, block=16384):
    """Row-by-row check of the DENSE (softmax) term of the Q-head gradients that the kernels output:
        g_E_out[j] = scale sum_b bf16(P[b,j]) hb[b]   (+ sum_{b: act[b]=j} coef[b] hb[b])
        g_b_out[j] = scale sum_b P[b,j]               (+ sum_{b: act[b]=j} coef[b])
        dH[b]      = scale sum_j bf16(P[b,j]) E_b[j]  (+ coef[b] E_b[act[b]])
    with P = exp(hb E_b^T + b_out - lse).  Every item row of g_E_out / g_b_out and every state row of dH is compared
    on its own, so a fault in a few rows cannot hide under the norm of the whole tensor (where the one-hot term
    dominates).  With (coef, act) the one-hot term is subtracted first, in float64.  Raises AssertionError naming the
    worst rows (with their 256- and 128-item group / 64- and 32-state stage indices); returns {output: worst err/sigma}.

    Noise model, per output element y = scale sum_k P_k x_k (k: states for the item side, items for dH; x = hb or E_b):
    * bf16 rounding of P.  The kernels round P to bf16 (RNE) before the product MFMA: qde2 / qde3 / qde_kernel and the
      QM_BWD_* modes of the skeleton at the true scale (exp(S + b - lse)); the fused forward (qfwd2 / qfwd3 and QM_LSE_DH)
      relative to a reference m of its own (exp(S + b - m), a per-slice maximum or a running one), rescaled later by
      exp(m - lse).  bf16 keeps its relative precision at any scale in the fp32 exponent range, so in both cases
      bf16(P) = P (1 + e) with |e| <= 2^-8 and e spread over the ulp: standard deviation ~2^-9 of the value (between
      2^-9.8 and 2^-8.8 depending on the position in the binade).  Where the P_k of a sum are spread over many bf16
      ulps, the e_k are independent: 2^-9 sqrt(sum_k (P_k x_k)^2).  Where they are not -- P[b, j] of one item is
      nearly the same for every state when the item's scores hardly depend on the state (small embeddings, as at
      initialisation) -- the e_k are nearly EQUAL and add up coherently, to about e |y|: the random term misses that by a
      factor up to sqrt(n).  The coherent part is taken from the rounding at the true scale, computed exactly:
      c = sum_k (bf16(P_k) - P_k) x_k.  (At the true scale that is what the kernel's rounding gives, up to rare flips of
      elements within the fp32 error of a rounding midpoint; at a shifted scale the kernel's e_k differ from those of c
      but are random to the same degree.)  So
          sigma_bf16 = 2^-9 sqrt(sum_k (P_k x_k)^2) + |c|.
      g_b_out has no such term: every kernel sums the fp32 P, before the conversion.
    * fp32 arithmetic.  (a) The sums: an fp32 chain of n terms with partial sums s_i errs by about
      u sqrt(sum_i s_i^2) <= u sqrt(n) (|y| + sqrt(sum_k (P_k x_k)^2)) (coherent part + random-walk part; u = 2^-24);
      slabs, cut ranges and MFMA blocks only shorten the chains.  (b) The exponent: P is exp2 of an fp32 argument
      (S + b) log2e - lse log2e formed from fp32 roundings of magnitude <= `arg` (the largest |S + b| plus the largest
      |lse|; for qde2 / qde3 the -lse log2e of the ABI is converted back to natural units, for the fused forward the
      weights exp(m - lse) add one more such argument), and v_exp_f32 adds ~1 ulp: relative P error <= u (2 arg + 4),
      bounded like (a).  Together
          sigma_fp32 = u (sqrt(n) + 2 arg + 4) (|y| + sqrt(sum_k (P_k x_k)^2)).
    * one-hot subtraction: the kernel's fp32 total was rounded after each of the cnt one-hot additions (and the final
      store): u (cnt + 2) (sum |one-hot terms| + |y|).
    The check is ||err_row|| <= K ||sigma_row|| + 1e-30 with sigma = scale (sigma_bf16 + sigma_fp32) (+ one-hot term).
    (A coherent sum at a shifted scale whose true-scale rounding happens to cancel, |c| ~ 0, is not covered: it needs
    a state whose P[b, :] all sit within one bf16 ulp of each other, which the bias spread of every case here rules out.)
    The reference shares the kernels' bf16 operands and lse, so nothing else separates the two."""
    if ref is None:
        ref = softmax_grad_reference(hb, lse, E_b, b_out, scale, items=g_E_out is not None or g_b_out is not None,
                                     states=dH is not None)
    sc = ref.scale
    B, Nn = ref.n_states, ref.n_items
    H = np.asarray(hb, dtype=np.float32).astype(np.float64)
    E = np.asarray(E_b, dtype=np.float32)
    if coef is not None:
        coef = np.asarray(coef, dtype=np.float32).astype(np.float64)
        act = np.asarray(act, dtype=np.int64)
        ua, inv = np.unique(act, return_inverse=True)
        cnt = np.bincount(inv, minlength=ua.size)
    report, fails = {}, []
    if g_E_out is not None:
        c_item = _fp32_coef(B, ref.arg)
        got = np.array(g_E_out, dtype=np.float64).reshape(Nn, -1)
        extra = None
        if coef is not None:
            oh = np.zeros((ua.size, H.shape[1]))
            oha = np.zeros_like(oh)
            np.add.at(oh, inv, coef[:, None] * H)
            np.add.at(oha, inv, np.abs(coef[:, None] * H))
            got[ua] -= oh
            extra = (ua, cnt, oha)
        for lo in range(0, Nn, block):
            hi = min(Nn, lo + block)
            y = sc * ref.dE[lo:hi]
            t = sc / _T_SHIFT * np.sqrt(ref.tE[lo:hi].astype(np.float64))
            sig = _BF16_SD * t + sc * np.abs(ref.cE[lo:hi]) + c_item * (np.abs(y) + t)
            if extra is not None:
                m = (extra[0] >= lo) & (extra[0] < hi)
                r = extra[0][m] - lo
                sig[r] += _U32 * (extra[1][m] + 2)[:, None] * (extra[2][m] + np.abs(y[r]))
            fails += _row_verdict("g_E_out", got[lo:hi] - y, sig, K, (256, 128), report, lo)
    if g_b_out is not None:
        c_item = _fp32_coef(B, ref.arg)
        got = np.array(g_b_out, dtype=np.float64).reshape(Nn)
        y = sc * ref.db
        sig = c_item * (np.abs(y) + sc / _T_SHIFT * np.sqrt(ref.tb))
        if coef is not None:
            oh = np.zeros(ua.size)
            oha = np.zeros(ua.size)
            np.add.at(oh, inv, coef)
            np.add.at(oha, inv, np.abs(coef))
            got[ua] -= oh
            sig[ua] += _U32 * (cnt + 2) * (oha + np.abs(y[ua]))
        fails += _row_verdict("g_b_out", got - y, sig, K, (256, 128), report)
    if dH is not None:
        c_state = _fp32_coef(Nn, ref.arg)
        got = np.array(dH, dtype=np.float64).reshape(B, -1)
        y = sc * ref.dH
        t = sc / _T_SHIFT * np.sqrt(ref.tH.astype(np.float64))
        sig = _BF16_SD * t + sc * np.abs(ref.cH) + c_state * (np.abs(y) + t)
        if coef is not None:
            oh = coef[:, None] * E[act].astype(np.float64)
            got -= oh
            sig += _U32 * 2.0 * (np.abs(oh) + np.abs(y))
        fails += _row_verdict("dH", got - y, sig, K, (64, 32), report)
    if fails:
        raise AssertionError("softmax gradient rows off: " + "; ".join(fails))
    return report


def qde_geometry(B, N, d, n_cu=256):
    """(form, G, T, W, grid, cut) of the long item-side backward kernel for a batch of B states, N items, width d -- the
    arithmetic of qde_plan and QdePieces::any_cut (csrc/qde_pieces.h), restated (tests/test_step_phase_geometry_cpu.py
    holds it to hand-worked rows and to that C code itself).
      form   qde2 (d = 128, B % 64 = 0), qde3 (d = 256, B % 32 = 0), else the generic qde_kernel<d>
      G      item groups: 256 items (8 waves x 32), 128 for d = 256 (4 waves)
      T      stages: 64 states, 32 for d = 256;  W = G T stage-units
      grid   min(W, n_cu): one persistent block per CU; block p works on stage-units [p W / grid, (p + 1) W / grid)
      cut    some block starts inside a group (p W / grid is no multiple of T for a p in [1, grid)): the piece of a group
             that does not hold stage 0 goes to a slab, and a fix-up (a launch, or the item-side Adam through CqlAdamFix)
             adds the slabs to the gradient rows.
    n_cu: the device's CU count as the library reads it (anything outside 1..256 counts as 256)."""
    assert d in (64, 128, 256) and B > 0 and N > 0
    if n_cu <= 0 or n_cu > 256:
        n_cu = 256
    if d == 128 and B % 64 == 0:
        form = "qde2"
    elif d == 256 and B % 32 == 0:
        form = "qde3"
    else:
        form = f"qde_kernel<{d}>"
    items = 32 * (4 if d == 256 else 8)
    ti = 32 if d == 256 else 64
    G, T = (N + items - 1) // items, (B + ti - 1) // ti
    W = G * T
    grid = min(W, n_cu)
    cut = any((p * W // grid) % T != 0 for p in range(1, grid))
    return form, G, T, W, grid, cut


def check_step_against_oracle(core, lay, theta, target, csr, seed, step, B, L, loss=None, gamma=0.99, alpha=1.0, tag="step"):
    """The intermediates and gradients that `core` holds after the forward + backward of `step` (before its update)
    against the float64 oracle run from the parameters (theta, target: flat fp32 numpy, layout `lay`) the step started
    from, on the log csr = (offsets, items, rewards): the sampled transitions exactly, the forward values within P3,
    every gradient segment normwise, the padding untouched, and the softmax part of the Q-head gradients row by row from
    the step's own states, lse, coef and actions (the one-hot term dominates the norms).  loss: the step's device loss."""
    off, items, rew = csr
    Nn = lay.n_items
    v = core.views(step)
    pos = O.sample_positions(seed, step, 0, B, int(off[-1]))
    users, tpos = O.positions_to_transitions(pos, off)
    out = O.loss_and_grads(lay, theta, target, off, items, rew, users, tpos, L, gamma, alpha)
    assert np.array_equal(v["users"].cpu().numpy(), users) and np.array_equal(v["tpos"].cpu().numpy(), tpos)
    np.testing.assert_allclose(v["h0_s"].cpu().numpy(), out.h0_s, rtol=1e-5, atol=1e-6)
    # bf16 state vectors: identical up to one bf16 ulp on rare rounding ties of an fp32 sum
    for name, ref in (("hb_s", out.hb_s), ("hb_sn", out.hb_sn)):
        got = bf16_to_np(v[name])
        print(f"STEPCHECK {tag} B={B} N={Nn} d={lay.d} {name}: {int(np.sum(got != ref))} of {got.size} bf16 values differ")
        assert np.mean(got != ref) < 2e-3
        np.testing.assert_allclose(got, ref, rtol=1e-2, atol=1e-3)
    np.testing.assert_allclose(v["q_a"].cpu().numpy(), out.q_a, atol=1e-3)          # P3 |dQ| <= 1e-3
    np.testing.assert_allclose(v["lse"].cpu().numpy(), out.lse, atol=1e-3)
    np.testing.assert_allclose(v["q_targ"].cpu().numpy(), out.q_targ, atol=1e-3)
    np.testing.assert_allclose(v["y"].cpu().numpy(), out.y, atol=1e-3)
    bad = O.argmax_margin_violations(v["a_star"].cpu().numpy(), out.a_star, out.qn_max, out.hb_sn,
                                     lay.view(O.shadow(theta), "E_out"), lay.view(theta, "b_out"),
                                     hb_got=bf16_to_np(v["hb_sn"]))
    assert bad.size == 0, bad                                                    # per row, P3 margin rule
    if loss is not None:
        assert abs(loss.item() - out.loss) < 1e-3 * abs(out.loss)
    assert rel_err(v["dH"].cpu().numpy(), out.dH) < 5e-3
    assert rel_err(v["dh0"].cpu().numpy(), out.dh0) < 5e-3
    g = core.grads.cpu().numpy()
    for nm in ("E_in", "E_out", "b_out", "W1", "b1", "W2", "b2"):
        assert rel_err(lay.view(g, nm), lay.view(out.grads, nm)) < 5e-3, nm
    # padding and the PAD row never receive gradient
    mask = np.ones(lay.total, bool)
    for nm in ("E_in", "E_out", "b_out", "W1", "b1", "W2", "b2"):
        mask[lay.off[nm]: lay.off[nm] + int(np.prod(lay.shape(nm)))] = False
    assert np.all(g[mask] == 0) and np.all(lay.view(g, "E_in")[Nn] == 0)
    # the softmax part of the Q-head gradients row by row, from the step's own states, lse, coef and actions (the
    # one-hot term dominates the norms above)
    rep = softmax_grad_rows(bf16_to_np(v["hb_s"]), v["lse"].cpu().numpy(), lay.view(O.shadow(theta), "E_out"),
                            lay.view(theta, "b_out"), np.float32(alpha / B), g_E_out=lay.view(g, "E_out"),
                            g_b_out=lay.view(g, "b_out"), dH=v["dH"].cpu().numpy(), coef=v["coef"].cpu().numpy(),
                            act=v["act"].cpu().numpy())
    print(f"ROWCHECK {tag} B={B} N={Nn} d={lay.d} " + " ".join(f"{k}={x:.3f}" for k, x in rep.items()))
    return rep


def topk_rule_violations(idx, val, cnt, Q, k, set_tol=1e-4, val_tol=1e-3):
    """P3 for a block of top-k lists against the reference score matrix Q (rows = the same users, inadmissible items at
    -inf), PER ROW: the count of admissible items, descending order, every reported score within val_tol of the
    reference's score of that item, and the set equal to the reference's outside a set_tol margin around the k-th
    reference score (an item in one list only must score within set_tol of it).  Returns (rows that violate it,
    number of boundary swaps over the passing rows)."""
    bad, swaps = [], 0
    ar = np.arange(Q.shape[1])
    for u in range(Q.shape[0]):
        order = np.lexsort((ar, -Q[u].astype(np.float64)))[:k]
        rv = Q[u][order]
        c = int(np.isfinite(rv).sum())
        ok = int(cnt[u]) == c and np.all(np.diff(val[u, :c]) <= 0)
        if ok and c:
            got = idx[u, :c].astype(np.int64)
            ok = (np.unique(got).size == c and got.min() >= 0 and
                  np.all(np.abs(val[u, :c] - Q[u, got]) <= val_tol))
            if ok:
                diff = set(got.tolist()) ^ set(order[:c].tolist())
                ok = all(abs(float(Q[u, j]) - float(rv[c - 1])) < set_tol for j in diff)
                swaps += len(diff) // 2
        if not ok:
            bad.append(u)
    return np.asarray(bad, dtype=np.int64), swaps


TOPK_IDX_SENTINEL, TOPK_VAL_SENTINEL, TOPK_CNT_SENTINEL = -77, 12345.0, -5


class TopkDevice:
    """One top-K problem on the device, for several cqlrec_score_topk calls (other k, with / without item_ids): the
    candidate rows E_c / b_c as the kernel gets them, ids = their global ids (None: candidate row = id), seen =
    (offsets int64, ascending global ids int32) with seen_rows (None: row u is user u's)."""

    def __init__(self, lib, Hb, E_c, b_c, ids=None, seen=None, seen_rows=None):
        self.lib, self.n_users, self.d = lib, Hb.shape[0], Hb.shape[1]
        self.n_cand = E_c.shape[0]
        self.H, self.E, self.b = bf16_dev(Hb), bf16_dev(E_c), dev(np.asarray(b_c, dtype=np.float32))
        self.ids = None if ids is None else dev(np.asarray(ids, dtype=np.int32))
        self.so = self.si = self.rows = self.seen_form = None
        if seen is not None:
            self.so = dev(np.asarray(seen[0], dtype=np.int64))
            self.si = dev(np.concatenate([np.asarray(seen[1], dtype=np.int32), np.zeros(1, np.int32)]))
            self.rows = None if seen_rows is None else dev(np.asarray(seen_rows, dtype=np.int32))

    def run(self, k, use_ids=True, guard_bytes=0, phases=None, query_form=False):
        """(idx, val, cnt) as numpy.  Outputs are pre-filled with sentinels, so an entry the pass left unwritten shows;
        guard_bytes > 0: a poisoned region right behind the declared workspace size must come back intact.
        phases: the CQLREC_TOPK_* phases of cqlrec_score_topk_phase to run in that order on the (fresh) workspace instead
        of cqlrec_score_topk; query_form: self.seen_form = what cqlrec_topk_seen_form says of that workspace afterwards
        (-1 without asking when the problem has no seen CSR: the function reports the word that the seen phase leaves in
        the workspace, and no seen phase ran, so the word was never written)."""
        nb = int(self.lib.cqlrec_topk_ws_bytes(self.n_users, self.n_cand, self.d, k))
        ws = ws_bytes_tensor(nb + guard_bytes)
        if guard_bytes:
            ws[nb:] = 0xFF                         # "every item seen" if a live row ever read it as bitmap
        out_idx = torch.full((self.n_users, k), TOPK_IDX_SENTINEL, dtype=torch.int32, device=DEV)
        out_val = torch.full((self.n_users, k), TOPK_VAL_SENTINEL, dtype=torch.float32, device=DEV)
        out_cnt = torch.full((self.n_users,), TOPK_CNT_SENTINEL, dtype=torch.int32, device=DEV)
        args = (ptr(self.H), self.n_users, ptr(self.E), ptr(self.b), self.n_cand, self.d, ptr(self.ids) if use_ids else None,
                ptr(self.so), ptr(self.si), ptr(self.rows), k, ptr(ws), nb, ptr(out_idx), ptr(out_val), ptr(out_cnt))
        if phases is None:
            N.check(self.lib.cqlrec_score_topk(*args, stream()))
        else:
            for phase in phases:
                N.check(self.lib.cqlrec_score_topk_phase(*args, phase, stream()))
        sync()
        if query_form and self.so is None:
            self.seen_form = -1
        elif query_form:
            form = ctypes.c_int32(-2)
            N.check(self.lib.cqlrec_topk_seen_form(ptr(ws), self.n_users, self.n_cand, self.d, k, ctypes.byref(form), stream()))
            self.seen_form = form.value
        if guard_bytes:
            assert bool((ws[nb:] == 0xFF).all()), "the pass wrote behind the workspace size it asked for"
        return out_idx.cpu().numpy(), out_val.cpu().numpy(), out_cnt.cpu().numpy()


def topk_case(lib, n_users, Nn, d, k, dyadic, seed, with_seen, cand=None, guard_bytes=0):
    Hb, Eb, b = qhead_inputs(n_users, Nn, d, dyadic, seed)
    rng = np.random.default_rng(seed)
    ids = np.arange(Nn, dtype=np.int32) if cand is None else cand
    E_c, b_c = Eb[ids], b[ids]
    Q = O.qvalues(Hb, E_c, b_c)
    seen_off = seen_items = None
    if with_seen:
        cnts = rng.integers(0, 40, n_users)
        cnts[0] = 0
        seen_off = np.zeros(n_users + 1, dtype=np.int64)
        np.cumsum(cnts, out=seen_off[1:])
        rows = []
        for u in range(n_users):
            top = np.argsort(-Q[u])[: cnts[u] // 2]                   # half of the seen items are the best ones
            rnd = rng.integers(0, Nn, cnts[u] - len(top))
            row = np.unique(np.concatenate([ids[top], rnd]).astype(np.int32))
            rows.append(row)
            seen_off[u + 1] = seen_off[u] + len(row)
        seen_items = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
        pos_of = -np.ones(Nn, dtype=np.int64)
        pos_of[ids] = np.arange(len(ids))
        for u in range(n_users):
            p = pos_of[seen_items[seen_off[u]: seen_off[u + 1]]]
            Q[u, p[p >= 0]] = -np.inf
    kk = min(k, len(ids))
    idx_c, val_ref = O.topk_rows(Q, kk)
    idx_ref = np.where(np.isfinite(val_ref), ids[idx_c], -1)
    case = TopkDevice(lib, Hb, E_c, b_c, ids=None if cand is None else ids,
                      seen=None if seen_off is None else (seen_off, seen_items))
    out_idx, out_val, out_cnt = case.run(k, guard_bytes=guard_bytes)
    return out_idx, out_val, out_cnt, idx_ref, val_ref, Q


# ---- top-K certificate against float64 ---------------------------------------------------------------------------------
# The blanket "1e-4 around the k-th score" rule above is ~3 000 ulp at |score| = 0.5 and unusable for large scores.  The
# certificate's only slack is eps, the worst-case bound of ANY fp32 summation order of the d products and the bias:
#     eps[u, c] = (d + 1) 2^-24 (sum_i |Hb[u,i] Eb[c,i]| + |b[c]|)
# (products of two bf16 values are exact in fp32; every one of the d additions rounds by at most 2^-24 of a partial sum
# that is itself at most (1 + 2^-24)^d times the sum of the absolute terms).  tests/test_topk_certificate_cpu.py is what
# justifies it: three fp32 orders accepted (they stay below 0.1 eps), every listed fault rejected.
TOPK_CERT_BLOCK = 64 * 262144          # float64 elements of the largest users x items block the certificate holds
TOPK_KINDS = ("plain", "neg", "straddle", "wide")


def topk_inputs(kind, n_users, Nn, d, seed, k_ref=16):
    """bf16-rounded (Hb, Eb) and an fp32 bias of the non-dyadic input kinds of the top-K tests:
    plain     qhead_inputs(..., dyadic=False)
    neg       plain, b -= 40: every score negative
    straddle  plain, b shifted so that the k_ref-th best score changes sign across users (median of them at 0)
    wide      plain, every E row scaled by exp(1.5 N(0,1)): group maxima spread over many exponents
    and, beside TOPK_KINDS (for the one-pass d = 128 kernels, whose running k-th best gates a slow path):
    ramp      plain, b += 0.05 item id: the running k-th best keeps being beaten all through the pass
    down      plain, b -= 0.05 item id: the bound is final after the first items; nothing later may enter"""
    Hb, Eb, b = qhead_inputs(n_users, Nn, d, False, seed)
    if kind in ("ramp", "down"):
        step = np.float32(0.05 if kind == "ramp" else -0.05)
        b = (b + step * np.arange(Nn, dtype=np.float32)).astype(np.float32)
    elif kind == "neg":
        b = (b - np.float32(40.0)).astype(np.float32)
    elif kind == "wide":
        s = np.exp(1.5 * np.random.default_rng(seed + 1).standard_normal(Nn)).astype(np.float32)
        Eb = O.bf16_round(Eb * s[:, None])
    elif kind == "straddle":
        Q = Hb @ Eb.T + b
        kk = min(k_ref, Nn)
        kth = -np.partition(-Q, kk - 1, axis=1)[:, kk - 1]
        b = (b - np.float32(np.median(kth))).astype(np.float32)
    elif kind != "plain":
        raise ValueError(kind)
    return Hb, Eb, b


def tk_geometry(n_cand, k):
    """(kernel, KPL, CB, tg, ngroups) of the two-pass family for n_cand candidates at k -- the arithmetic of sel_groups
    (csrc/select_common.h, SEL_MAX_GROUPS = 4096) and TK_BY_KPL / TK_LAUNCH in csrc/topk.hip, restated (the tests assert their case tables against it)."""
    tiles = (n_cand + 31) // 32
    tg = 1
    while (tiles + tg - 1) // tg > 4096:
        tg *= 2
    ngroups = (tiles + tg - 1) // tg
    kpl = 16 if ngroups <= 1024 else (32 if ngroups <= 2048 else 64)
    if k <= 16:
        return "small", kpl, 0, tg, ngroups
    return "select", kpl, (1024 if k <= 512 else 4096), tg, ngroups


def tk2_geometry(n_users, n_cand, k, n_cu=256):
    """(kernel, KC, users_per_block, nsplit, split_rows) of the one-pass d = 128 family (item_ids = NULL, k <= 16) -- the
    arithmetic of cql_topk2_supported / cql_topk4_use (default mode) / cql_topk2_split in csrc/qhead_topk2.hip and
    qhead_topk4.hip, restated.  n_cu: the CU count the library reads from the device (256 on an MI355X)."""
    assert 1 <= k <= 16 and n_cand * 256 < 2 ** 31, "not a shape of the one-pass family"
    stages = (n_cand + 63) // 64
    four = n_users >= 512 * 160 and stages * 1024 < 2 ** 31
    upb = 512 if four else 256
    rblks = (n_users + upb - 1) // upb
    want = max(1, min((n_cu + rblks - 1) // rblks, stages // 8, 16))       # at least eight stages per slice, at most 16 slices
    split_rows = (stages + want - 1) // want * 64
    return "qtopk4" if four else "qtopk2", 10 if k <= 10 else 16, upb, (n_cand + split_rows - 1) // split_rows, split_rows


class TopkReference:
    """float64 scores and eps of one (Hb, Eb, b), one item chunk at a time; cached when the whole block is one chunk."""

    def __init__(self, Hb, Eb, b):
        self.H = np.asarray(Hb, dtype=np.float32).astype(np.float64)
        self.Ha = np.abs(self.H)
        self.E = np.asarray(Eb, dtype=np.float32)
        self.b = np.asarray(b, dtype=np.float32).astype(np.float64)
        self.n_users, self.d = self.H.shape
        self.n_cand = self.E.shape[0]
        self.step = max(1, TOPK_CERT_BLOCK // self.n_users)
        self._cache = None

    def blocks(self):
        """yields (lo, hi, Q64[:, lo:hi], eps[:, lo:hi]); the arrays must not be modified"""
        if self._cache is not None:
            yield self._cache
            return
        for lo in range(0, self.n_cand, self.step):
            hi = min(self.n_cand, lo + self.step)
            Ec = self.E[lo:hi].astype(np.float64)
            Q = self.H @ Ec.T
            Q += self.b[lo:hi]
            A = self.Ha @ np.abs(Ec).T
            A += np.abs(self.b[lo:hi])
            A *= (self.d + 1) * _U32
            blk = (lo, hi, Q, A)
            if lo == 0 and hi == self.n_cand:
                self._cache = blk
            yield blk


def _cert_where(u, cs, tg):
    cs = [int(c) for c in np.atleast_1d(cs)[:4]]
    return f"user {int(u)} [" + ", ".join(f"c {c} /32:{c // 32} /{32 * tg}:{c // (32 * tg)}" for c in cs) + "]"


def topk_certificate(idx, val, cnt, Hb, Eb, b, k, ids=None, seen=None, seen_rows=None, ref=None):
    """Certificate of a block of top-k lists against float64, from the kernels' own operands: Hb [n_users, d] and
    Eb [n_cand, d] bf16-rounded, b [n_cand] fp32 (candidate rows, compacted as the kernel got them); ids [n_cand]
    ascending global ids of the candidate rows (None: 0..n_cand-1); seen = (offsets, ascending global ids) CSR, row
    seen_rows[u] (None: u) is user u's.  Per user, with Q64 = Hb Eb^T + b in float64 and eps as above:
      1. cnt == min(k, number of admissible candidates)   (admissible: a candidate row whose id is not in the seen row)
      2. the first cnt ids are distinct and admissible; the rest of the row is exactly -1 / -inf
      3. |val[i] - Q64[idx[i]]| <= eps[idx[i]]
      4. the row is ordered by its own values, exactly: val non-increasing, ids ascending where values are equal
      5. (cnt == k) every admissible candidate c outside the row has Q64[c] - eps[c] <= val[cnt - 1]
    No excluded rows, no swap budget.  Raises AssertionError naming the worst users, their candidate rows and groups
    (c // 32 and c // (32 tg)).  Returns {"ratio": the largest |val - Q64| / eps, "share": the share of users whose
    k-th and (k+1)-th admissible float64 scores are closer than the sum of their eps -- the only place where (5) cannot
    see a dropped item; from the reference alone}."""
    idx = np.asarray(idx).astype(np.int64)
    val = np.asarray(val, dtype=np.float32)
    cnt = np.asarray(cnt).astype(np.int64)
    if ref is None:
        ref = TopkReference(Hb, Eb, b)
    n_users, n_cand = ref.n_users, ref.n_cand
    assert idx.shape == (n_users, k) and val.shape == (n_users, k) and cnt.shape == (n_users,)
    tg = tk_geometry(n_cand, k)[3]
    ids = np.arange(n_cand, dtype=np.int64) if ids is None else np.asarray(ids).astype(np.int64)
    assert ids.shape == (n_cand,) and (n_cand < 2 or np.all(np.diff(ids) > 0)), "ids must be ascending and distinct"
    # candidate rows excluded per user (ascending)
    seen_pos = [np.zeros(0, np.int64)] * n_users
    if seen is not None:
        off, items = np.asarray(seen[0]).astype(np.int64), np.asarray(seen[1]).astype(np.int64)
        rows = np.arange(n_users) if seen_rows is None else np.asarray(seen_rows).astype(np.int64)
        for u in range(n_users):
            s = items[off[rows[u]]: off[rows[u] + 1]]
            p = np.minimum(np.searchsorted(ids, s), n_cand - 1)
            seen_pos[u] = np.unique(p[ids[p] == s])                  # seen ids that are no candidates drop out
    n_adm = np.array([n_cand - len(p) for p in seen_pos], dtype=np.int64)
    fails = []

    # ---- 1, 2: counts, padding, ids ------------------------------------------------------------------------------------
    want = np.minimum(k, n_adm)
    bad = np.nonzero(cnt != want)[0]
    if bad.size:
        fails.append(f"(1) count: {bad.size} users, e.g. " +
                     "; ".join(f"user {u}: cnt {cnt[u]}, admissible {n_adm[u]}" for u in bad[:4]))
    c_ok = np.clip(cnt, 0, k)
    col = np.arange(k)[None, :]
    live = col < c_ok[:, None]
    pad_bad = np.nonzero((~live & ((idx != -1) | ~np.isneginf(val))).any(1))[0]
    if pad_bad.size:
        fails.append(f"(2) padding is not -1 / -inf: users {pad_bad[:6].tolist()}")
    pos = np.searchsorted(ids, np.where(live, idx, ids[0]))
    pos = np.minimum(pos, n_cand - 1)
    is_cand = live & (ids[pos] == idx)
    for u in np.nonzero((live & ~is_cand).any(1))[0][:4]:
        fails.append(f"(2) user {u}: ids outside the candidate set: {idx[u][live[u] & ~is_cand[u]][:4].tolist()}")
    for u in range(n_users):
        pu = pos[u][is_cand[u]]
        if np.unique(pu).size != pu.size:
            vals, c = np.unique(pu, return_counts=True)
            fails.append("(2) duplicated: " + _cert_where(u, vals[c > 1], tg))
        hit = pu[np.isin(pu, seen_pos[u])]
        if hit.size:
            fails.append("(2) seen items returned: " + _cert_where(u, hit, tg))

    # ---- 4: the row's own order ----------------------------------------------------------------------------------------
    vb = (val + np.float32(0.0)).view(np.uint32)
    both = live[:, 1:] & live[:, :-1]
    with np.errstate(invalid="ignore"):
        desc = val[:, 1:] > val[:, :-1]
    ties = (vb[:, 1:] == vb[:, :-1]) & (idx[:, 1:] <= idx[:, :-1])
    unordered = ~(val[:, 1:] <= val[:, :-1])                                      # also catches NaN
    for name, m in (("values ascend", both & (desc | unordered)), ("equal values, ids not ascending", both & ties)):
        for u in np.nonzero(m.any(1))[0][:4]:
            j = int(np.nonzero(m[u])[0][0])
            fails.append(f"(4) {name}: user {u} at rank {j}/{j + 1}: ids {idx[u, j]}, {idx[u, j + 1]} "
                         f"values {val[u, j]!r}, {val[u, j + 1]!r}")

    # ---- 3, 5 and the boundary share: one sweep over the item chunks ------------------------------------------------------
    q_sel = np.full((n_users, k), np.nan)
    e_sel = np.full((n_users, k), np.nan)
    full = (cnt == k) & (want == k)
    last = np.where(full, val[np.arange(n_users), np.clip(cnt - 1, 0, k - 1)].astype(np.float64), np.inf)
    left_n = np.zeros(n_users, np.int64)
    left_worst = np.full(n_users, -np.inf)
    left_c = np.zeros(n_users, np.int64)
    top_q = np.full((n_users, 0), -np.inf)
    top_e = np.zeros((n_users, 0))
    uu = np.arange(n_users)[:, None]
    for lo, hi, Q, A in ref.blocks():
        m = is_cand & (pos >= lo) & (pos < hi)
        ur, jr = np.nonzero(m)
        q_sel[ur, jr] = Q[ur, pos[ur, jr] - lo]
        e_sel[ur, jr] = A[ur, pos[ur, jr] - lo]
        adm = np.ones(Q.shape, dtype=bool)
        for u in range(n_users):
            p = seen_pos[u]
            adm[u, p[np.searchsorted(p, lo): np.searchsorted(p, hi)] - lo] = False
        Qa = np.where(adm, Q, -np.inf)
        # the k + 1 best admissible of the reference so far
        w = min(k + 1, hi - lo)
        part = np.argpartition(-Qa, w - 1, axis=1)[:, :w] if w < hi - lo else np.broadcast_to(np.arange(hi - lo), (n_users, hi - lo))
        top_q = np.concatenate([top_q, Qa[uu, part]], 1)
        top_e = np.concatenate([top_e, A[uu, part]], 1)
        if top_q.shape[1] > k + 1:
            o = np.argpartition(-top_q, k, axis=1)[:, :k + 1]
            top_q, top_e = top_q[uu, o], top_e[uu, o]
        # (5): admissible, not in the row, surely above the row's last value
        Qa[ur, pos[ur, jr] - lo] = -np.inf
        low = Qa - A
        over = low > last[:, None]
        n_over = over.sum(1)
        left_n += n_over
        for u in np.nonzero(n_over)[0]:
            c = int(np.argmax(np.where(over[u], low[u], -np.inf)))
            if low[u, c] - last[u] > left_worst[u]:
                left_worst[u], left_c[u] = low[u, c] - last[u], lo + c
    with np.errstate(invalid="ignore"):
        err = np.abs(val.astype(np.float64) - q_sel)
        ratio = np.where(is_cand, err / np.maximum(e_sel, 1e-300), 0.0)
        ratio = np.where(is_cand & (err == 0), 0.0, ratio)
        off3 = is_cand & ~(err <= e_sel)
    if off3.any():
        us = np.nonzero(off3.any(1))[0]
        us = us[np.argsort(-np.nan_to_num(ratio[us], nan=np.inf).max(1))][:4]
        fails.append(f"(3) values off by more than eps for {int(off3.any(1).sum())} users; worst: " + "; ".join(
            _cert_where(u, pos[u][off3[u]], tg) + f" err/eps {np.nan_to_num(ratio[u], nan=np.inf).max():.3g}" for u in us))
    if left_n.any():
        us = np.nonzero(left_n)[0]
        us = us[np.argsort(-left_worst[us])][:4]
        fails.append(f"(5) better items left out for {int((left_n > 0).sum())} users; worst: " + "; ".join(
            _cert_where(u, left_c[u], tg) + f" ({int(left_n[u])} items, Q64 - eps above the last value by "
            f"{left_worst[u]:.3g})" for u in us))
    share = 0.0
    if top_q.shape[1] >= k + 1:
        o = np.argsort(-top_q, axis=1, kind="stable")
        tq, te = top_q[uu, o], top_e[uu, o]
        with np.errstate(invalid="ignore"):
            close = np.isfinite(tq[:, k]) & (tq[:, k - 1] - tq[:, k] < te[:, k - 1] + te[:, k])
        share = float(close.mean())
    out = {"ratio": float(np.nanmax(ratio, initial=0.0)), "share": share}
    if fails:
        raise AssertionError(f"top-{k} certificate (n_cand {n_cand}, tg {tg}, boundary share {share:.3f}): " + " | ".join(fails))
    return out


# ---- case builders and bitwise comparisons shared by the top-K kernel tests (two-pass: test_gpu_topk_two_pass; one-pass
# d = 128: test_gpu_topk_onchip, test_topk_onchip_cases_cpu) ------------------------------------------------------------
BOOST_GROUPS = (5, 69, 133, 197, 261, 325)           # all owned by lane 5 of the selection wave (group = slot * 64 + lane)


def _np_topk(S, k, ids, seen_mask=None):
    """exact (score desc, id asc) top-k of fp32 scores; inadmissible entries masked; padded with -1 / -inf"""
    S = S.astype(np.float32).copy()
    if seen_mask is not None:
        S[seen_mask] = -np.inf
    kk = min(k, S.shape[1])
    order = np.argsort(-S, axis=1, kind="stable")[:, :kk]
    val = np.take_along_axis(S, order, 1)
    ok = np.isfinite(val)
    idx = np.full((S.shape[0], k), -1, np.int32)
    out = np.full((S.shape[0], k), -np.inf, np.float32)
    idx[:, :kk] = np.where(ok, ids[order], -1)
    out[:, :kk] = np.where(ok, val, -np.inf)
    return idx, out, ok.sum(1).astype(np.int32)


def _inputs(kind, n_users, n_cat, d, seed):
    if kind == "dyadic":
        return qhead_inputs(n_users, n_cat, d, True, seed)
    if kind in ("flat1", "flat3"):
        rng = np.random.default_rng(seed)
        Eb = qhead_inputs(1, n_cat, d, False, seed)[1]
        b = np.full(n_cat, 0.25, np.float32) if kind == "flat1" else \
            rng.choice(np.array([-1.5, 0.25, 2.0], np.float32), n_cat)          # no -0.0: it sorts below +0.0 here
        return np.zeros((n_users, d), np.float32), Eb, b.astype(np.float32)
    if kind == "plain+boost":
        return topk_inputs("plain", n_users, n_cat, d, seed)
    return topk_inputs(kind, n_users, n_cat, d, seed)


def _row(rng, best, n_cat, n_best, n_other):
    """n_best of the user's best candidates (global ids) + n_other other catalogue ids, ascending, exactly that long
    where the catalogue allows it"""
    top = best[:max(0, n_best)]
    pool = rng.choice(n_cat + 8, size=min(n_cat + 8, n_other + n_other // 2 + 16), replace=False)    # + 8: ids past the catalogue
    other = pool[~np.isin(pool, top)][:n_other]
    return np.unique(np.concatenate([top, other])).astype(np.int32)


def _seen_rows(rng, S, ids, n_cat):
    """(offsets, items), seen_rows, admissibility mask -- see the module docstring"""
    n_users, n_cand = S.shape
    n_rows = n_users + 7
    rows_of = rng.permutation(n_rows)[:n_users].astype(np.int32)
    if n_users > 2:
        rows_of[2] = rows_of[1]
    lens = {0: 0, 3: 1, 4: 511, 5: 512, 6: 513, 7: 3000}
    rows = [np.sort(rng.choice(n_cat, min(n_cat, 9), replace=False)).astype(np.int32) for _ in range(n_rows)]
    for u in range(n_users):
        if u == 2 and n_users > 2:
            continue
        best = ids[np.argsort(-S[u], kind="stable")]
        if u == 8:
            row = _row(rng, best, n_cat, n_cand - 40, 10)
        elif u == 9:
            row = _row(rng, best, n_cat, n_cand - 5, 10)
        elif u == 10:
            row = _row(rng, best, n_cat, n_cand, 10)
        else:
            ln = min(lens.get(u, int(rng.integers(0, 40))), n_cat)
            row = _row(rng, best, n_cat, ln // 2, ln - ln // 2)
        rows[rows_of[u]] = row
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    mask = np.stack([np.isin(ids, rows[rows_of[u]]) for u in range(n_users)])
    return (off, np.concatenate(rows).astype(np.int32)), rows_of, mask


def build_case(cid, d, n_cand, ids_mode, kind, n_users, with_seen):
    """host side of a case of the table: candidate rows as CQLCore.score_topk compacts them, seen CSR, admissibility"""
    seed = sum(map(ord, cid)) * 7 + d
    rng = np.random.default_rng(seed)
    n_cat = n_cand if ids_mode == "identity" else n_cand + n_cand // 4 + 17
    Hb, Eb, b = _inputs(kind, n_users, n_cat, d, seed)
    ids = np.arange(n_cand, dtype=np.int64) if ids_mode == "identity" else \
        np.sort(rng.choice(n_cat, n_cand, replace=False)).astype(np.int64)
    E_c, b_c = np.ascontiguousarray(Eb[ids]), b[ids].copy()
    if kind == "plain+boost":
        for g in BOOST_GROUPS:
            b_c[g * 32 + 3] += np.float32(10.0)
    S = (Hb @ E_c.T + b_c).astype(np.float32)
    seen = rows_of = mask = None
    if with_seen:
        seen, rows_of, mask = _seen_rows(rng, S, ids, n_cat)
    return dict(Hb=Hb, E_c=E_c, b_c=b_c, ids=ids, seen=seen, rows=rows_of, mask=mask, S=S, kind=kind, n_cat=n_cat)


def _oracle(c, k):
    Q = O.qvalues(c["Hb"], c["E_c"], c["b_c"])
    if c["mask"] is not None:
        Q[c["mask"]] = -np.inf
    kk = min(k, Q.shape[1])
    idx_c, v = O.topk_rows(Q, kk)
    ok = np.isfinite(v)
    idx = np.full((Q.shape[0], k), -1, np.int32)
    val = np.full((Q.shape[0], k), -np.inf, np.float32)
    idx[:, :kk] = np.where(ok, c["ids"][idx_c], -1)
    val[:, :kk] = np.where(ok, v, -np.inf)
    return idx, val, ok.sum(1).astype(np.int32)


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def _no_sentinel(res, what):
    idx, val, cnt = res
    assert not (idx == TOPK_IDX_SENTINEL).any() and not (val == np.float32(TOPK_VAL_SENTINEL)).any() and \
        not (cnt == TOPK_CNT_SENTINEL).any(), f"{what}: output entries left unwritten"


def _assert_same(a, b, what):
    assert np.array_equal(a[2], b[2]), f"{what}: counts differ for users {np.nonzero(a[2] != b[2])[0][:6].tolist()}"
    bad = np.nonzero((a[0] != b[0]).any(1) | (_bits(a[1]) != _bits(b[1])).any(1))[0]
    if bad.size:
        u = int(bad[0])
        j = int(np.nonzero((a[0][u] != b[0][u]) | (_bits(a[1][u]) != _bits(b[1][u])))[0][0])
        raise AssertionError(f"{what}: {bad.size} users differ, first user {u} at rank {j}: ids {a[0][u, j]} / {b[0][u, j]}, "
                             f"values {a[1][u, j]!r} / {b[1][u, j]!r}")


def _assert_prefix(short, long_, k2, what):
    want = (long_[0][:, :k2], long_[1][:, :k2], np.minimum(long_[2], k2))
    _assert_same(short, want, what)
