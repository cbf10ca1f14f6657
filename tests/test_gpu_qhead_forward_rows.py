"""The Q-head forward through the C ABI, ROW BY ROW against float64 (tests/qhead_forward_reference.py): the logsumexp of
every form inside a bound derived from the row's own data, the arg-max exact on dyadic data with crafted ties at every
boundary of the kernels' geometry, the derived margin rule on random data, masked (bias = -inf) items, and
cqlrec_gather_dot as bits on non-dyadic inputs.

Which form a shape reaches (qhead.hip: qhead_fwd_impl, cql_qhead_fwd_lse_dh; ports in the reference module, asserted per case):

  entry                               d     form                                    slices
  cqlrec_qhead_fwd LSE                any   QM_LSE skeleton ("fwd_lse")             fwd_split(rows, N)
  cqlrec_qhead_fwd ARGMAX             64    QM_ARGMAX skeleton, 64-item stages      fwd_split(rows, N)
  cqlrec_qhead_fwd ARGMAX             128   qargmax2, 64-item stages of two tiles   qargmax2_split(rows, N)
  cqlrec_qhead_fwd ARGMAX             256   qargmax2, 32-item stages, two register  qargmax2_split(rows, N)
                                            sets by stage parity
  cqlrec_qhead_fwd_lse_dh             64    QM_LSE_DH skeleton ("fused_generic")    fused_split(rows, N, d)
  cqlrec_qhead_fwd_lse_dh             128   qfwd2; on overflow of a partial sum     fused_split
                                            (bias "+200", N > 40) the guarded
                                            "fused_generic" redoes the pass
  cqlrec_qhead_fwd_lse_dh             256   qfwd3; the same fall-back               fused_split (half the target)
  (the d = 128 skeleton ARGMAX is launched by the training step only: test_gpu_step_forward_rows.py; the d = 256
  skeleton ARGMAX needs n_items * 512 >= 2^31 and is out of reach of any test)

  N = 1100 and 4099 give qargmax2 2 and 8 slices of 576 items (9 / 18 stages each), the skeleton 8 and 32 slices."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from oracle import cql_oracle as O
from replay_cql_amd import _native as N

import pairs_reference as PR
import qhead_forward_reference as R
from helpers import DEV, bf16_dev, dev, ptr, qhead_inputs, release_kept, stream, sync, ws_bytes_tensor

pytestmark = pytest.mark.gpu

LSE_SHAPES = [(1, 5), (1, 33), (32, 64), (33, 65), (255, 257), (257, 4099), (300, 5003), (1024, 20011)]
DIMS = (64, 128, 256)


@pytest.fixture(scope="module")
def lib():
    return N.load()


class Device:
    """one (H, E, b) on the device and the three forward entries on it"""

    def __init__(self, lib, H, E, b):
        self.lib, (self.rows, self.d), self.n = lib, H.shape, E.shape[0]
        self.H, self.E, self.b = bf16_dev(H), bf16_dev(E), dev(np.asarray(b, np.float32))
        self.nb = int(lib.cqlrec_qhead_ws_bytes(self.rows, self.n, self.d))
        self.ws = ws_bytes_tensor(self.nb)

    def set_items(self, E, b):
        self.E.copy_(torch.as_tensor(O.bf16_bits(E).astype(np.int16)).view(torch.bfloat16))
        self.b.copy_(torch.as_tensor(np.asarray(b, np.float32)))

    def _fwd(self, mode, want_idx, want_n2):
        val = torch.full((self.rows,), float("nan"), device=DEV)
        idx = torch.full((self.rows,), -7, dtype=torch.int32, device=DEV) if want_idx else None
        n2 = torch.full((self.rows,), float("nan"), device=DEV) if want_n2 else None
        N.check(self.lib.cqlrec_qhead_fwd(ptr(self.H), self.rows, ptr(self.E), ptr(self.b), self.n, self.d, mode, ptr(self.ws),
                                          self.nb, ptr(val), ptr(idx), ptr(n2), stream()))
        sync()
        return val.cpu().numpy(), None if idx is None else idx.cpu().numpy(), None if n2 is None else n2.cpu().numpy()

    def lse(self):
        v, _, n2 = self._fwd(N.QHEAD_LSE, False, True)
        return v, n2

    def argmax(self):
        v, i, _ = self._fwd(N.QHEAD_ARGMAX, True, False)
        return i, v

    def fused_lse(self):
        nb = int(self.lib.cqlrec_qhead_fused_ws_bytes(self.rows, self.n, self.d))
        ws = ws_bytes_tensor(nb)
        lse = torch.full((self.rows,), float("nan"), device=DEV)
        n2 = torch.full((self.rows,), float("nan"), device=DEV)
        N.check(self.lib.cqlrec_qhead_fwd_lse_dh(ptr(self.H), self.rows, ptr(self.E), ptr(self.b), self.n, self.d, ptr(ws), nb,
                                                 ptr(lse), ptr(n2), stream()))
        sync()
        return lse.cpu().numpy(), n2.cpu().numpy()


def _nlse2_bits(lse):
    return (-lse * R.LOG2E32).astype(np.float32).view(np.uint32)


def _fused_name(d, Nn, ref):
    first = R.fused_form(d, Nn)
    if first == "generic":
        return "fused_generic"
    return "fused_generic" if ref.overflow[first] else first


def _check_both_lse(dv, ref, d, Nn, tag):
    """both lse entries of one device case against one reference; returns the worst ratios"""
    lse, n2 = dv.lse()
    w1 = R.check_lse(lse, ref, "fwd_lse")
    assert np.array_equal(n2.view(np.uint32), _nlse2_bits(lse)), "nlse2 is not the fp32 product -lse * log2e"
    name = _fused_name(d, Nn, ref)
    lse, n2 = dv.fused_lse()
    w2 = R.check_lse(lse, ref, name)
    assert np.array_equal(n2.view(np.uint32), _nlse2_bits(lse)), "nlse2 is not the fp32 product -lse * log2e (fused)"
    print(f"ROWCHECK lse fwd_lse {tag} worst={w1:.3f}")
    print(f"ROWCHECK lse {name} {tag} worst={w2:.3f}")
    return name


# ---- lse, every form, per row inside bound_lse -------------------------------------------------------------------------
@lru_cache(maxsize=1)
def _lse_ref(B, Nn, d, bias):
    H, E, b, _ = R.lse_inputs(B, Nn, d, bias)
    return R.LseReference(H, E, b, R.lse_forms(B, Nn, d))


@pytest.mark.parametrize("bias", ["none", "ramp", "+200"])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("B,Nn", LSE_SHAPES)
def test_lse_rows(lib, B, Nn, d, bias):
    H, E, b, _ = R.lse_inputs(B, Nn, d, bias)
    ref = _lse_ref(B, Nn, d, bias)
    name = _check_both_lse(Device(lib, H, E, b), ref, d, Nn, f"B={B} N={Nn} d={d} bias={bias}")
    # the form the table promises: the fall-back exactly where the step of +200 lies behind a slice's first tile
    falls_back = bias == "+200" and Nn > 40 and d != 64
    assert name == ("fused_generic" if d == 64 or falls_back else R.fused_form(d, Nn))
    release_kept()


# ---- masked items ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["scattered", "first_tile"])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("B,Nn", [(33, 65), (257, 4099)])
def test_masked_items(lib, B, Nn, d, mask):
    H, E, b, _ = R.lse_inputs(B, Nn, d, "none")
    b = b.copy()
    rng = np.random.default_rng(Nn + d)
    dead = rng.random(Nn) < 0.1
    if mask == "first_tile":
        dead[:32] = True                  # qfwd2 / qfwd3: nothing finite in the slice's first tile, the reference is 0
    dead[Nn - 1] = False
    b[dead] = -np.inf
    ref = R.LseReference(H, E, b, R.lse_forms(B, Nn, d))
    dv = Device(lib, H, E, b)
    name = _check_both_lse(dv, ref, d, Nn, f"B={B} N={Nn} d={d} masked={mask}")
    assert name == ("fused_generic" if d == 64 else R.fused_form(d, Nn))
    imax, vmax = dv.argmax()
    assert not dead[imax].any(), "the arg-max is a masked item"
    w = R.check_argmax(H, E, b, imax, vmax)
    print(f"ROWCHECK argmax masked={mask} B={B} N={Nn} d={d} worst={w:.3f}")
    release_kept()


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("B,Nn", [(33, 65), (70, 1100)])
def test_nothing_finite_in_a_row(lib, B, Nn, d):
    """every item masked: lse = -inf (not NaN), vmax = -inf, imax = 0, as qhead_argmax_resolve_kernel promises"""
    H, E, b, _ = R.lse_inputs(B, Nn, d, "none")
    dv = Device(lib, H, E, np.full(Nn, -np.inf, np.float32))
    for lse, n2 in (dv.lse(), dv.fused_lse()):
        assert np.isneginf(lse).all(), lse[:4]
        assert np.isposinf(n2).all(), n2[:4]
    imax, vmax = dv.argmax()
    assert np.isneginf(vmax).all() and (imax == 0).all()
    release_kept()


# ---- arg-max ------------------------------------------------------------------------------------------------------------
AM_ROWS = (1, 256, 257)
AM_N = (33, 64, 65, 1000, 1100, 4099)


def _assert_argmax_form(d, rows, Nn):
    form, stage, nsplit, split_rows = R.argmax_geometry(d, rows, Nn)
    assert form == ("skeleton" if d == 64 else "qargmax2")
    if Nn in (1100, 4099):
        assert nsplit >= 2 and split_rows < Nn, "a slice-boundary case without a slice boundary"
    if form == "qargmax2" and Nn == 1100:
        assert nsplit == 2 and split_rows // stage >= 8
    return stage, split_rows


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("Nn", AM_N)
@pytest.mark.parametrize("rows", AM_ROWS)
def test_argmax_dyadic_exact_with_ties(lib, rows, Nn, d):
    stage, split_rows = _assert_argmax_form(d, rows, Nn)
    H, E, b = R.dyadic_inputs(rows, Nn, d, seed=rows * 13 + Nn + d)
    dv = Device(lib, H, E, b)
    cases = [("plain", 0, 0, E, b, None)]
    for f, g in R.tie_positions(stage, 32, split_rows, Nn, parity=(d == 256)):
        for pattern in R.TIE_PATTERNS:
            E2, b2, want = R.tie_layout(E, b, pattern, f, g)
            cases.append((pattern, f, g, E2, b2, want))
    for pattern, f, g, E2, b2, want in cases:
        idx_ref, val_ref = R.exact_argmax(H, E2, b2)
        if want is not None:
            assert (idx_ref == want).all()
        dv.set_items(E2, b2)
        imax, vmax = dv.argmax()
        assert np.array_equal(imax.astype(np.int64), idx_ref), (pattern, f, g, np.nonzero(imax != idx_ref)[0][:4], imax[:4])
        assert np.array_equal(vmax.view(np.uint32), val_ref.view(np.uint32)), (pattern, f, g)
    release_kept()


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("Nn", AM_N)
@pytest.mark.parametrize("rows", AM_ROWS)
def test_argmax_random_rows(lib, rows, Nn, d):
    _assert_argmax_form(d, rows, Nn)
    H, E, b = qhead_inputs(rows, Nn, d, False, rows * 17 + Nn + d)
    imax, vmax = Device(lib, H, E, b).argmax()
    w = R.check_argmax(H, E, b, imax, vmax)
    print(f"ROWCHECK argmax rows={rows} N={Nn} d={d} worst={w:.3f}")
    release_kept()


# ---- gather_dot on non-dyadic inputs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("rows", [1, 77, 4099])
def test_gather_dot_bits(lib, rows, d):
    Nn = 300
    H, E, b = qhead_inputs(rows, Nn, d, False, rows + d)
    idx = np.random.default_rng(rows).integers(0, Nn, rows).astype(np.int32)
    idx[: min(rows, 9)] = idx[0]                                   # repeated indices
    out = torch.full((rows,), float("nan"), device=DEV)
    N.check(lib.cqlrec_gather_dot(ptr(bf16_dev(H)), ptr(bf16_dev(E)), ptr(dev(b)), ptr(dev(idx)), rows, d, ptr(out), stream()))
    sync()
    ref = PR.gather_dot(O.bf16_bits(H), O.bf16_bits(E), b, np.arange(rows), idx)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    release_kept()
