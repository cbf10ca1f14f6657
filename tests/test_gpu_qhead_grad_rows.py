"""The softmax part of the Q-head gradients, ROW BY ROW (helpers.softmax_grad_rows), for every form the dispatch
picks: the item-side kernels (qde2, qde3, the generic qde_kernel<64|128|256>, with and without stream-K cut ranges and
their fix-up), the state side of the backward (the QM_BWD_DH skeleton) and the fused forward (qfwd2, qfwd3, the generic
QM_LSE_DH skeleton, its guarded fall-back) + dh_finish.  Each case runs with coef = 0 (every row is pure softmax term)
and with a realistic coef (the checker subtracts the one-hot term), through the C ABI.

The normwise checks of test_gpu_kernels.py cannot see a wrong tail group, two swapped rows, a dropped stage or a wrong
lse row: the one-hot rows dominate their norm.  Here every item row of g_E_out / g_b_out and every state row of dH is
held to its own rounding-noise scale."""
import numpy as np
import pytest
import torch

from replay_cql_amd import _native as N

from helpers import (DEV, bf16_dev, dev, ptr, softmax_grad_reference, softmax_grad_rows, stream, sync,
                     ws_bytes_tensor)

pytestmark = pytest.mark.gpu

LOG2E = np.float32(1.4426950408889634)


@pytest.fixture(scope="module")
def lib():
    return N.load()


def _inputs(B, Nn, d, seed, bias="none"):
    """bf16 states mixing flat (small norm) and peaked (large norm) softmax rows in one batch, bf16 item table, fp32 bias
    ("ramp": grows with the item id, so a running reference keeps being beaten; "+200": a step of +200 nats behind the
    first 40 items, so a reference fixed from the first tile overflows), a realistic coef = (delta - alpha) / B with
    alpha = 1 and duplicate actions."""
    from oracle import cql_oracle as O
    rng = np.random.default_rng(seed)
    amp = rng.choice([0.05, 0.5, 3.0, 8.0], size=B).astype(np.float32)
    H = O.bf16_round(rng.standard_normal((B, d)).astype(np.float32) * amp[:, None])
    E = O.bf16_round((rng.standard_normal((Nn, d)) / np.sqrt(d)).astype(np.float32))
    b = (rng.standard_normal(Nn) * 0.3).astype(np.float32)
    if bias == "ramp":
        b = (b + 0.02 * np.arange(Nn, dtype=np.float32)).astype(np.float32)
    elif bias == "+200":
        b[40:] += np.float32(200.0)
    coef = ((rng.standard_normal(B).astype(np.float32) - np.float32(1.0)) / np.float32(B)).astype(np.float32)
    act = rng.integers(0, Nn, B).astype(np.int32)
    act[: min(B, 8)] = act[0]
    return H, E, b, coef, act


def _lse64(H, E, b):
    lse = np.empty(H.shape[0])
    for lo in range(0, H.shape[0], 256):
        Q = H[lo:lo + 256].astype(np.float64) @ E.T.astype(np.float64) + b
        m = Q.max(1)
        lse[lo:lo + 256] = m + np.log(np.exp(Q - m[:, None]).sum(1))
    return lse


def _report(tag, rep):
    print(f"ROWCHECK {tag} " + " ".join(f"{k}={v:.3f}" for k, v in rep.items()))


# ---- item side (and the state side of the backward) ---------------------------------------------------------------
# n_cu = 256; the rows are helpers.qde_geometry's (test_step_phase_geometry_cpu.py).  Item-side form (qde_pieces.h: qde_plan; W = G * T stage-units, grid =
# min(W, 256), a range starts inside a group ("cut", slab + fix-up) when some p * W / grid is not a multiple of T):
#   B     N      d    form                               G x T = W        grid  cut
#   64    5003   128  qde2 (B % 64 = 0)                  20 x 1 = 20      20    no (T = 1)
#   1024  20011  128  qde2                               79 x 16 = 1264   256   yes (stream-K)
#   1000  20011  128  qde_kernel<128> (B % 64 != 0)      79 x 16 = 1264   256   yes
#   100   1000   128  qde_kernel<128>                    4 x 2 = 8        8     yes (grid = W and T > 1)
#   512   5003   256  qde3 (B % 32 = 0)                  40 x 16 = 640    256   yes
#   500   5003   256  qde_kernel<256> (B % 32 != 0)      40 x 16 = 640    256   yes
#   1024  20011  64   qde_kernel<64> (8 waves)           79 x 16 = 1264   256   yes
#   128   100    128  qde2, N < 128                      1 x 2 = 2        2     yes (block 1 starts at stage 1)
#   1     3001   128  qde_kernel<128>, B = 1             12 x 1 = 12      12    no
#   1     777    256  qde_kernel<256>, B = 1             7 x 1 = 7        7     no
# (groups: 256 items for qde2 and the 8-wave qde_kernel, 128 for d = 256; stages: 64 states, 32 for d = 256.)  Every N
# but 100 leaves a partial last group.  The state side (QM_BWD_DH skeleton) runs at the same shapes.
ITEM_SHAPES = [(64, 5003, 128), (1024, 20011, 128), (1000, 20011, 128), (100, 1000, 128), (512, 5003, 256),
               (500, 5003, 256), (1024, 20011, 64), (128, 100, 128), (1, 3001, 128), (1, 777, 256)]


@pytest.mark.parametrize("B,Nn,d", ITEM_SHAPES)
def test_qhead_bwd_rows(lib, B, Nn, d):
    H, E, b, coef, act = _inputs(B, Nn, d, seed=B * 7 + Nn + d)
    lse = _lse64(H, E, b)
    nlse2 = (-lse * LOG2E).astype(np.float32)
    lse_k = -nlse2.astype(np.float64) * np.log(2.0)            # the lse the kernels work with
    scale = np.float32(1.0 / B)
    ref = softmax_grad_reference(H, lse_k, E, b, scale)
    Hd, Ed, bd, nd, ad = bf16_dev(H), bf16_dev(E), dev(b), dev(nlse2), dev(act)
    nb = int(lib.cqlrec_qhead_bwd_ws_bytes(B, Nn, d))
    ws = ws_bytes_tensor(nb)

    def outs():
        return (torch.full((B, d), 7.0, dtype=torch.float32, device=DEV),      # every element must be overwritten
                torch.full((Nn, d), 7.0, dtype=torch.float32, device=DEV),
                torch.full((Nn,), 7.0, dtype=torch.float32, device=DEV))

    # coef = 0: the two halves, separately
    zero = dev(np.zeros(B, np.float32))
    dH, gE, gb = outs()
    N.check(lib.cqlrec_qhead_bwd_items(ptr(Hd), ptr(nd), ptr(zero), ptr(ad), B, ptr(Ed), ptr(bd), Nn, d, float(scale),
                                       ptr(ws), nb, ptr(gE), ptr(gb), stream()))
    N.check(lib.cqlrec_qhead_bwd_states(ptr(Hd), ptr(nd), ptr(zero), ptr(ad), B, ptr(Ed), ptr(bd), Nn, d, float(scale),
                                        ptr(ws), nb, ptr(dH), stream()))
    sync()
    rep = softmax_grad_rows(H, lse_k, E, b, scale, g_E_out=gE.cpu().numpy(), g_b_out=gb.cpu().numpy(),
                            dH=dH.cpu().numpy(), ref=ref)
    _report(f"bwd_halves coef=0 B={B} N={Nn} d={d}", rep)
    # realistic coef: the whole backward
    dH, gE, gb = outs()
    N.check(lib.cqlrec_qhead_bwd(ptr(Hd), ptr(nd), ptr(dev(coef)), ptr(ad), B, ptr(Ed), ptr(bd), Nn, d, float(scale),
                                 ptr(ws), nb, ptr(dH), ptr(gE), ptr(gb), stream()))
    sync()
    rep = softmax_grad_rows(H, lse_k, E, b, scale, g_E_out=gE.cpu().numpy(), g_b_out=gb.cpu().numpy(),
                            dH=dH.cpu().numpy(), coef=coef, act=act, ref=ref)
    _report(f"bwd coef B={B} N={Nn} d={d}", rep)


# ---- fused forward + dh_finish (the training step's dH) --------------------------------------------------------------
# State-side form of cqlrec_qhead_fwd_lse_dh (cql_qfwd2_supported: d = 128; cql_qfwd3_supported: d = 256; otherwise the
# QM_LSE_DH mode of the skeleton with its running reference; slices from qs_choose_split):
#   B     N      d    bias   form
#   1000  20011  128  -      qfwd2 (per-slice fixed reference)
#   300   4099   128  ramp   qfwd2, reference beaten by later tiles (P > 1, still finite)
#   300   4099   128  +200   qfwd2 overflows -> flag -> guarded QM_LSE_DH fall-back redoes the pass
#   512   5003   256  -      qfwd3
#   300   4099   256  ramp   qfwd3
#   300   4099   256  +200   qfwd3 overflows -> guarded fall-back
#   1024  20011  64   -      QM_LSE_DH skeleton (running reference)
#   300   4099   64   ramp   QM_LSE_DH, rescale path taken often
#   1     3001   128  -      qfwd2, B = 1
FUSED_SHAPES = [(1000, 20011, 128, "none"), (300, 4099, 128, "ramp"), (300, 4099, 128, "+200"),
                (512, 5003, 256, "none"), (300, 4099, 256, "ramp"), (300, 4099, 256, "+200"),
                (1024, 20011, 64, "none"), (300, 4099, 64, "ramp"), (1, 3001, 128, "none")]


@pytest.mark.parametrize("B,Nn,d,bias", FUSED_SHAPES)
def test_fused_forward_dh_rows(lib, B, Nn, d, bias):
    H, E, b, coef, act = _inputs(B, Nn, d, seed=B * 5 + Nn + d + len(bias), bias=bias)
    scale = np.float32(1.0 / B)
    nb = int(lib.cqlrec_qhead_fused_ws_bytes(B, Nn, d))
    ws = ws_bytes_tensor(nb)
    Hd, Ed, bd, ad = bf16_dev(H), bf16_dev(E), dev(b), dev(act)
    lse_d = torch.empty(B, dtype=torch.float32, device=DEV)
    N.check(lib.cqlrec_qhead_fwd_lse_dh(ptr(Hd), B, ptr(Ed), ptr(bd), Nn, d, ptr(ws), nb, ptr(lse_d), None, stream()))
    outs = []
    for cf in (np.zeros(B, np.float32), coef):
        dH = torch.full((B, d), 7.0, dtype=torch.float32, device=DEV)
        N.check(lib.cqlrec_qhead_dh_finish(ptr(ws), B, Nn, d, ptr(lse_d), ptr(dev(cf)), ptr(ad), ptr(Ed), float(scale),
                                           ptr(dH), stream()))
        outs.append(dH)
    sync()
    lse_k = lse_d.cpu().numpy()
    assert np.isfinite(lse_k).all()
    np.testing.assert_allclose(lse_k, _lse64(H, E, b), rtol=2e-6, atol=2e-5)
    ref = softmax_grad_reference(H, lse_k, E, b, scale, items=False)
    rep = softmax_grad_rows(H, lse_k, E, b, scale, dH=outs[0].cpu().numpy(), ref=ref)
    _report(f"fused coef=0 B={B} N={Nn} d={d} bias={bias}", rep)
    rep = softmax_grad_rows(H, lse_k, E, b, scale, dH=outs[1].cpu().numpy(), coef=coef, act=act, ref=ref)
    _report(f"fused coef B={B} N={Nn} d={d} bias={bias}", rep)
