"""The bits behind the cut of the item-side backward (csrc/qde_pieces.h), pinned to the commit BEFORE that header existed:
SHA-256 digests of g_E_out / g_b_out and of theta, both Adam moments, the target net and both bf16 shadows after the
update, against tests/golden/qde_cut_known_answers.json -- recorded by `python tests/test_gpu_qde_cut_known_answers.py
--record` from a build of that commit (CQLREC_LIB), on the CU count the file names.  The geometry of a cut depends on the
CU count, so on another count the test FAILS with that message; it does not skip.

Shapes: the six that head tests/test_step_phase_geometry_cpu.py::ROWS, the smallest that reach each (form, cut); N = 1000
and N = 5003 leave a last group partly past n_items.  Each goes through the three routes to the gradient:
  items    cqlrec_qhead_bwd_items: long kernel, fix-up LAUNCH, one-hot part (the entry point always passes accumulate = 0;
           no entry point of the library reaches the long kernels' accumulate = 1 branch)
  steps    cqlrec_train_steps, 3 steps: the deferred fix inside the item-side Adam launch
  phased   the phased entry points: 3 steps as CQLCore.train_steps(phased=True) drives them, then a 4th by hand whose
           gradient is digested between backward and update (early long kernel, one-hot part, deferred fix-up launch)
Inputs come from integer hashing and IEEE multiply / add only, so they do not depend on a library's random streams or
transcendentals."""
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from replay_cql_amd import _native as N  # noqa: E402
from replay_cql_amd.core import CQLCore, CQLHyper  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = ROOT / "tests" / "golden" / "qde_cut_known_answers.json"
DEV = "cuda:0"
WINDOW = 8
# (B, N, d): qde2 / generic / qde3 / generic d = 64 / qde2 uncut (T = 1) / qde2 with W > grid
SHAPES = [(128, 1000, 128), (96, 1000, 128), (64, 1000, 256), (128, 2000, 64), (64, 5003, 128), (1024, 5003, 128)]
STATE = ("theta", "adam_m", "adam_v", "target", "theta_b", "target_b")


def key(shape):
    return "B{}-N{}-d{}".format(*shape)


def _hash(n, seed):
    """n 64-bit hashes (splitmix64 of seed-offset counters): integer arithmetic only"""
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x632BE59BD9B4E019)
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _unit(n, seed):
    """n float32 in [-1, 1): 24 hash bits each, exact"""
    return ((_hash(n, seed) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)).astype(np.float32)


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _bf16(x):
    return torch.as_tensor(x).to(DEV).to(torch.bfloat16).contiguous()


def route_items(lib, shape):
    """cqlrec_qhead_bwd_items on hashed inputs: small scores, -lse near -ln N, a one-hot part on every state"""
    B, Nn, d = shape
    seed = B * 7 + Nn + d
    H = _bf16((_unit(B * d, seed) * np.float32(0.25)).reshape(B, d))
    E = _bf16((_unit(Nn * d, seed + 1) * np.float32(0.25)).reshape(Nn, d))
    b = torch.as_tensor(_unit(Nn, seed + 2) * np.float32(0.05)).to(DEV)
    ln_n = {1000: 6.9, 2000: 7.6, 5003: 8.5}[Nn]
    nlse2 = torch.as_tensor((np.float32(-ln_n) + _unit(B, seed + 3) * np.float32(0.1)) * np.float32(1.4426950408889634)).to(DEV)
    coef = torch.as_tensor(_unit(B, seed + 4) * np.float32(1.0 / B)).to(DEV)
    # one action per item at most (7 is coprime to every N here, B <= N): this entry point adds the one-hot part with
    # atomics, and two states on one row would leave the order of their sum to the scheduler
    act = torch.as_tensor(((np.arange(B, dtype=np.int64) * 7 + 3) % Nn).astype(np.int32)).to(DEV)
    assert B <= Nn and Nn % 7 != 0
    nb = int(lib.cqlrec_qhead_bwd_ws_bytes(B, Nn, d))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    gE = torch.full((Nn, d), 7.0, dtype=torch.float32, device=DEV)          # every element must be overwritten
    gb = torch.full((Nn,), 7.0, dtype=torch.float32, device=DEV)
    N.check(lib.cqlrec_qhead_bwd_items(H.data_ptr(), nlse2.data_ptr(), coef.data_ptr(), act.data_ptr(), B, E.data_ptr(),
                                       b.data_ptr(), Nn, d, float(np.float32(1.0 / B)), ws.data_ptr(), nb, gE.data_ptr(),
                                       gb.data_ptr(), torch.cuda.current_stream().cuda_stream), "qhead_bwd_items")
    torch.cuda.synchronize()
    return {"g_E_out": _sha(gE), "g_b_out": _sha(gb)}


def _core(shape):
    """a context on hashed parameters (target net apart from theta, non-zero biases) and a hashed log of 300 users"""
    B, Nn, d = shape
    core = CQLCore(Nn, CQLHyper(d=d, window=WINDOW, batch=B, seed=12), device=DEV)
    lay = core.layout
    theta = np.zeros(int(lay.total), np.float32)
    for i, (name, amp) in enumerate((("E_in", 0.1), ("E_out", 0.1), ("b_out", 0.05), ("W1", 0.08), ("b1", 0.05), ("W2", 0.08),
                                     ("b2", 0.05))):
        shp = lay.shape(name)
        n = (Nn if name == "E_in" else shp[0]) * (shp[1] if len(shp) > 1 else 1)      # the PAD row of E_in stays 0
        theta[lay.offset(name): lay.offset(name) + n] = _unit(n, 100 + i) * np.float32(amp)
    target = (theta + _unit(theta.size, 200) * np.float32(0.01) * (theta != 0)).astype(np.float32)
    core.load_flat(theta, target)
    U = 300
    lens = (5 + _hash(U, 300) % np.uint64(30)).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(off[-1])
    core.set_log(off, (_hash(nnz, 301) % np.uint64(Nn)).astype(np.int32), (_unit(nnz, 302) * np.float32(0.5) + np.float32(0.5)))
    return core


def _state(core):
    return {n: _sha(getattr(core, n)) for n in STATE}


def route_steps(shape):
    core = _core(shape)
    core.train_steps(3)
    torch.cuda.synchronize()
    return _state(core)


def route_phased(lib, shape):
    core = _core(shape)
    core.train_steps(3, phased=True)
    torch.cuda.synchronize()
    out = {"after_3": _state(core)}
    # a 4th step by hand: the long kernel launched early on an item-side stream, its cut pieces added by backward_items
    c, lay = core._train_ctx(), core.layout
    ref, main, aux = C.byref(c), torch.cuda.current_stream(), N.aux_stream(0)
    ev = torch.cuda.Event()
    N.check(lib.cqlrec_train_step_forward_early_items(ref, 3, None, main.cuda_stream, None, aux.cuda_stream), "forward")
    ev.record(main)
    N.check(lib.cqlrec_train_step_backward_rest(ref, 3, main.cuda_stream), "backward_rest")
    aux.wait_event(ev)
    N.check(lib.cqlrec_train_step_backward_items(ref, 3, aux.cuda_stream), "backward_items")
    torch.cuda.synchronize()
    g = core.grads
    out["g_E_out"] = _sha(g[int(lay.off_E_out): int(lay.off_E_out) + core.n_items * core.hyper.d])
    out["g_b_out"] = _sha(g[int(lay.off_b_out): int(lay.off_b_out) + core.n_items])
    N.check(lib.cqlrec_train_step_update(ref, 3, main.cuda_stream), "update")
    torch.cuda.synchronize()
    out["after_4"] = _state(core)
    return out


def measure(lib, shape):
    return {"items": route_items(lib, shape), "steps": route_steps(shape), "phased": route_phased(lib, shape)}


@pytest.fixture(scope="module")
def golden():
    g = json.loads(GOLDEN.read_text())
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert g["n_cu"] == n_cu, (f"tests/golden/qde_cut_known_answers.json was recorded on {g['n_cu']} CUs, this device has "
                               f"{n_cu}: the cut falls elsewhere, the digests cannot match")
    return g


def test_golden_file_covers_the_shapes(golden):
    assert sorted(golden["shapes"]) == sorted(key(s) for s in SHAPES)


@pytest.mark.parametrize("shape", SHAPES, ids=key)
def test_digests_are_the_recorded_ones(golden, shape):
    got, want = measure(N.load(), shape), golden["shapes"][key(shape)]
    for route in ("items", "steps", "phased"):
        print(f"QDECUT {key(shape)} {route}: " + ("same" if got[route] == want[route] else f"{got[route]} / {want[route]}"))
    assert got == want


if __name__ == "__main__" and "--record" in sys.argv:
    lib_ = N.load()
    GOLDEN.write_text(json.dumps({"n_cu": torch.cuda.get_device_properties(0).multi_processor_count,
                                  "shapes": {key(s): measure(lib_, s) for s in SHAPES}}, indent=1) + "\n")
    print(GOLDEN)
