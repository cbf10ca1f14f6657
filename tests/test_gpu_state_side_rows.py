"""The state-side kernels of the step, element by element against float64: encoder backward at its block and chunk edges
and with dead ReLU rows, the TD / loss kernel at every batch size around its 256-thread block, the bf16 cast that makes
the shadows of every loaded model, and the Adam launch at a size where its capped grid strides.

Bounds are the derived ones of scatter_reference.py ((n + 2) u sum |t_i|, propagated through rounded intermediates);
bit-exact where the operation is (the cast, Adam, y of a terminal transition)."""
import functools

import numpy as np
import pytest
import torch

from oracle import cql_oracle as O
from replay_cql_amd import _native as N

import scatter_reference as R
from helpers import DEV, bf16_dev, bf16_to_np, dev, ptr, stream, sync, ws_bytes_tensor

pytestmark = pytest.mark.gpu

BF16_MIN = O.bf16_from_bits(np.array([1], dtype=np.uint16))[0]        # smallest positive bf16: 2^-133


@pytest.fixture(scope="module")
def lib():
    return N.load()


# ------------------------------------------------------------------------------------------------ encoder backward
@functools.lru_cache(maxsize=None)
def _enc_weights(d):
    rng = np.random.default_rng(100 + d)
    return tuple(O.bf16_round((rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)) for _ in range(2))


ENC_ROWS = [(rows, d) for d in (64, 128, 256) for rows in (1, 31, 32, 33, 127, 128, 129, 300)] + [(4103, 128)]


@pytest.mark.parametrize("rows,d", ENC_ROWS)
def test_encoder_bwd_rows(lib, rows, d):
    """rows at the 32-row block edge of enc_bwd_dx_kernel, at the 128-row chunk edge of enc_bwd_dw_kernel, 1, and the
    step's own 4096 + 7.  z_b holds exact +0, -0 and the smallest positive bf16 (alive); about one row in eight is dead
    (z_b <= 0 throughout: zeros of both signs and negative values) and must give dh0 = 0 exactly.  Outputs are pre-filled
    with NaN: an element the kernels leave unwritten fails its bound."""
    rng = np.random.default_rng(7 * d + rows)
    dH = rng.standard_normal((rows, d)).astype(np.float32)
    zb = O.bf16_round(np.maximum(rng.standard_normal((rows, d)), 0).astype(np.float32))
    dead = np.arange(rows) % 8 == 3
    zb[dead] = np.where(rng.random((int(dead.sum()), d)) < 0.5, np.float32(-0.0),
                        -O.bf16_round(np.abs(rng.standard_normal((int(dead.sum()), d))).astype(np.float32)))
    zb[dead, ::5] = 0.0
    live_row = int(np.flatnonzero(~dead)[-1])
    zb[live_row, :3] = (0.0, -0.0, BF16_MIN)
    assert np.array_equal(O.bf16_bits(zb[live_row, :3]), [0x0000, 0x8000, 0x0001])
    h0b = O.bf16_round(rng.standard_normal((rows, d)).astype(np.float32))
    W1b, W2b = _enc_weights(d)
    nb = int(lib.cqlrec_encoder_bwd_ws_bytes(rows, d))
    ws = ws_bytes_tensor(nb)
    nan = float("nan")
    out = {"gW1": torch.full((d, d), nan, device=DEV), "gb1": torch.full((d,), nan, device=DEV),
           "gW2": torch.full((d, d), nan, device=DEV), "gb2": torch.full((d,), nan, device=DEV),
           "dh0": torch.full((rows, d), nan, device=DEV)}
    N.check(lib.cqlrec_encoder_bwd(ptr(dev(dH)), ptr(bf16_dev(zb)), ptr(bf16_dev(h0b)), ptr(bf16_dev(W1b)),
                                   ptr(bf16_dev(W2b)), rows, d, ptr(ws), nb, ptr(out["gW1"]), ptr(out["gb1"]),
                                   ptr(out["gW2"]), ptr(out["gb2"]), ptr(out["dh0"]), stream()))
    sync()
    ref, dead_ref = R.encoder_bwd_reference(dH, zb, h0b, W1b, W2b)
    assert np.array_equal(dead_ref, dead)
    report, fails = {}, []
    got = {nm: t.cpu().numpy() for nm, t in out.items()}
    for nm, (r, b) in ref.items():
        fails += R.element_check(nm, got[nm], r, b, report)
    print(f"SCATTERCHECK encoder_bwd rows={rows} d={d} " + R.fmt_report(report))
    assert not fails, fails
    assert np.all(got["dh0"][dead] == 0), "a dead row has a gradient"


# ------------------------------------------------------------------------------------------------ TD target / loss
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 1000, 4096, 5003])
def test_td_loss_rows(lib, B):
    rng = np.random.default_rng(B)
    q_a, lse, qt, rew = [rng.standard_normal(B).astype(np.float32) for _ in range(4)]
    lse = (lse + 5).astype(np.float32)
    done = (rng.random(B) < 0.3).astype(np.float32)
    if B >= 2:
        done[0], done[1] = 1.0, 0.0
    term = done == 1.0
    qt[term] = (np.where(rng.random(int(term.sum())) < 0.5, -1.0, 1.0) * 1e30 *
                (1 + rng.random(int(term.sum())))).astype(np.float32)          # must not leak into a terminal target
    gamma, alpha, inv = 0.99, 0.7, 1.0 / (2 * B)
    d_in = [dev(x) for x in (q_a, lse, qt, rew, done)]

    def run(want_y, want_loss):
        coef = torch.full((B,), float("nan"), device=DEV)
        y = torch.full((B,), float("nan"), device=DEV) if want_y else None
        loss = torch.full((1,), float("nan"), device=DEV) if want_loss else None
        N.check(lib.cqlrec_td_loss(*[ptr(t) for t in d_in], B, gamma, alpha, inv, ptr(coef), ptr(y), ptr(loss), stream()))
        sync()
        return coef, y, loss
    coef, y, loss = run(True, True)
    ref = R.td_reference(q_a, lse, qt, rew, done, gamma, alpha, inv)
    report = {}
    fails = R.element_check("y", y.cpu().numpy(), *ref["y"], report)
    fails += R.element_check("coef", coef.cpu().numpy(), *ref["coef"], report)
    fails += R.element_check("loss", loss.cpu().numpy()[0], *ref["loss"], report)
    print(f"SCATTERCHECK td_loss B={B} " + R.fmt_report(report))
    assert not fails, fails
    assert np.array_equal(y.cpu().numpy()[term].view(np.uint32), rew[term].view(np.uint32)), "y != rew at done == 1"
    # the forms the header allows give the same coefficients; two calls the same bits
    for want_y, want_loss in ((False, True), (True, False), (False, False), (True, True)):
        c2, y2, l2 = run(want_y, want_loss)
        assert torch.equal(c2.view(torch.int32), coef.view(torch.int32)), (want_y, want_loss)
        if want_y:
            assert torch.equal(y2.view(torch.int32), y.view(torch.int32))
        if want_loss:
            assert torch.equal(l2.view(torch.int32), loss.view(torch.int32))


# ------------------------------------------------------------------------------------------------ bf16 cast
def _cast(lib, x_bits):
    """uint32 fp32 bit patterns (padded with +0 to a multiple of 4) -> uint16 bf16 bit patterns from the device"""
    n = x_bits.size
    pad = (-n) % 4
    src = torch.as_tensor(np.concatenate([x_bits, np.zeros(pad, np.uint32)]).view(np.int32)).to(DEV)
    dst = torch.full((n + pad,), 0x7FFF, dtype=torch.int16, device=DEV)          # a NaN pattern: unwritten shows
    N.check(lib.cqlrec_cast_bf16(ptr(src), ptr(dst), n + pad, stream()))
    sync()
    return dst.cpu().numpy().view(np.uint16)[:n]


def _oracle_bits(x_bits):
    return O.bf16_bits(x_bits.view(np.float32))


def test_cast_bf16_ties_and_edges(lib):
    """every rounding tie of the binade [1, 2) with both parities of the kept bit, and their neighbours one fp32 ulp
    below and above, in both signs; the largest finite fp32 values (round to infinity); +-0 and +-inf"""
    hi = (np.arange(128, dtype=np.uint32) << 16) | np.uint32(0x3F800000)
    ties = np.concatenate([hi | np.uint32(0x8000), hi | np.uint32(0x7FFF), hi | np.uint32(0x8001)])
    ties = np.concatenate([ties, ties | np.uint32(0x80000000)])
    top = np.array([0x7F7FFFFF, 0x7F7F8000, 0x7F7F8001, 0x7F7F7FFF, 0x7F7F0000, 0x7F7E8000], dtype=np.uint32)
    top = np.concatenate([top, top | np.uint32(0x80000000)])
    edges = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000], dtype=np.uint32)
    x = np.concatenate([ties, top, edges])
    want = _oracle_bits(x)
    assert np.array_equal(want[:128], (hi >> 16) + (np.arange(128) & 1))        # ties go to the even neighbour
    assert np.array_equal(want[768:772], [0x7F80, 0x7F80, 0x7F80, 0x7F7F])      # the largest values round to +inf
    assert np.array_equal(want[-4:], [0x0000, 0x8000, 0x7F80, 0xFF80])
    got = _cast(lib, x)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(int(x[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]]


def test_cast_bf16_nan_stays_nan(lib):
    x = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F808000, 0x7FBFFFFF],
                 dtype=np.uint32)
    got = _cast(lib, x)
    assert np.all((got & 0x7FFF) > 0x7F80), [hex(int(g)) for g in got]


def test_cast_bf16_subnormals(lib):
    """fp32 subnormal inputs round like everything else (no flush): to a bf16 subnormal, to zero below half of the
    smallest one (ties to even), to the smallest normal from the top of the range -- what the oracle gives (P1)"""
    rng = np.random.default_rng(4)
    x = np.concatenate([np.array([0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00010000, 0x00018000, 0x00028000,
                                  0x007F7FFF, 0x007F8000, 0x007FFFFF, 0x00400000], dtype=np.uint32),
                        rng.integers(1, 1 << 23, 493).astype(np.uint32)])
    x = np.concatenate([x, x | np.uint32(0x80000000)])
    want = _oracle_bits(x)
    assert np.array_equal(want[:11], [0, 0, 0, 1, 1, 2, 2, 0x7F, 0x80, 0x80, 0x40])
    got = _cast(lib, x)
    print("SCATTERCHECK cast_bf16 subnormals: device " + " ".join(f"{int(v):04x}" for v in got[:11]) +
          " oracle " + " ".join(f"{int(v):04x}" for v in want[:11]) + f" mismatches={int((got != want).sum())} of {x.size}")
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(int(x[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]]


def test_cast_bf16_large_buffer_strides(lib):
    """8 388 916 elements = 4 (8192 x 256 + 77): the grid is capped at 8192 blocks, so 77 threads take a second trip"""
    n = 4 * (8192 * 256 + 77)
    rng = np.random.default_rng(6)
    x = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    expo = (x >> 23) & np.uint32(0xFF)
    x = np.where((expo == 0) | (expo == 255), (x & np.uint32(0x807FFFFF)) | np.uint32(0x3F000000), x)   # normal, finite
    got = _cast(lib, x)
    want = _oracle_bits(x)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, [(int(i), hex(int(x[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]])
    assert np.array_equal(got[-308:], want[-308:])


def test_cast_bf16_bad_sizes_raise(lib):
    t = torch.zeros(16, dtype=torch.float32, device=DEV)
    o = torch.zeros(16, dtype=torch.int16, device=DEV)
    for n in (0, 1, 2, 3, 5, 14, -4):
        with pytest.raises(N.CqlrecError, match="multiple of 4"):
            N.check(lib.cqlrec_cast_bf16(ptr(t), ptr(o), n, stream()))
    sync()
    assert torch.count_nonzero(o).item() == 0


# ------------------------------------------------------------------------------------------------ Adam
def test_adam_bit_exact_beyond_one_grid_round(lib):
    """test_adam_bit_exact's comparison at n = 4 (8192 x 256 + 77): the launch caps the grid at 8192 blocks of 256
    threads, one float4 each per trip, so the last 308 elements are reached only by the grid-stride loop's second trip"""
    n = 4 * (8192 * 256 + 77)
    rng = np.random.default_rng(11)
    theta = rng.standard_normal(n, dtype=np.float32)
    target = theta + rng.standard_normal(n, dtype=np.float32) * np.float32(0.01)
    m = rng.standard_normal(n, dtype=np.float32) * np.float32(0.01)
    v = rng.random(n, dtype=np.float32) * np.float32(1e-4)
    g = rng.standard_normal(n, dtype=np.float32) * np.float32(0.1)
    g[:100] = 0
    v[:50] = 0
    m[:50] = 0
    theta0_tail = theta[-308:].copy()
    d_th, d_g, d_m, d_v, d_t = dev(theta), dev(g), dev(m), dev(v), dev(target)
    d_thb = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    d_tb = torch.empty_like(d_thb)
    t = 3
    step_size, sqrt_bc2 = O.adam_scalars(t, 1e-3, 0.9, 0.999)
    N.check(lib.cqlrec_adam_ema(ptr(d_th), ptr(d_g), ptr(d_m), ptr(d_v), ptr(d_t), ptr(d_thb), ptr(d_tb), n,
                                float(step_size), float(sqrt_bc2), 0.9, 0.999, 1e-8, 0.005, 0, stream()))
    sync()
    with np.errstate(all="ignore"):
        O.adam_ema_step(theta, g, m, v, target, t, 1e-3)
    assert np.array_equal(d_th.cpu().numpy(), theta)
    assert np.array_equal(d_m.cpu().numpy(), m)
    assert np.array_equal(d_v.cpu().numpy(), v)
    assert np.array_equal(d_t.cpu().numpy(), target)
    assert np.array_equal(bf16_to_np(d_thb), O.bf16_round(theta))
    assert np.array_equal(bf16_to_np(d_tb), O.bf16_round(target))
    # the elements beyond a whole round of the grid were updated ...
    tail = d_th[-308:].cpu().numpy()
    assert np.array_equal(tail, theta[-308:]) and np.all(tail != theta0_tail)
    assert torch.count_nonzero(d_g[-308:]).item() == 308                      # zero_grads = 0 left them
    # ... and zero_grads = 1 clears them
    N.check(lib.cqlrec_adam_ema(ptr(d_th), ptr(d_g), ptr(d_m), ptr(d_v), ptr(d_t), ptr(d_thb), ptr(d_tb), n, 1e-3, 1.0,
                                0.9, 0.999, 1e-8, 0.005, 1, stream()))
    sync()
    assert torch.count_nonzero(d_g.view(torch.int32)).item() == 0
