"""The training-step workspace, byte for byte: cqlrec_train_ws_bytes and the 17 views of cqlrec_train_views_get (offsets
from the workspace base) for steps 0..3, against tests/golden/train_ws_layout_known_answers.json.

Both queries are host-only and dereference nothing, so the ctx holds made-up non-NULL pointers and a made-up workspace
base; no GPU.  The file was recorded by `python tests/test_train_ws_layout_cpu.py --record` from a build of the commit
BEFORE the step driver was split (train.hip as one file, carve_step called per part): it pins the layout that refactor
had to keep, and every later one."""
import ctypes as C
import json
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from replay_cql_amd import _native as N  # noqa: E402
from replay_cql_amd import build as B  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "train_ws_layout_known_answers.json"
WS_BASE = 1 << 40
STEPS = (0, 1, 2, 3)
# (batch, n_items, d, window): the shapes of tests/test_gpu_step_phases.py::SHAPES at its window, the two timed
# configurations, and the smallest legal one
SHAPES = [(128, 1000, 128, 8), (96, 1000, 128, 8), (64, 1000, 256, 8), (128, 2000, 64, 8), (64, 5003, 128, 8),
          (1024, 5003, 128, 8), (4096, 100000, 128, 50), (4096, 1000000, 256, 50), (1, 1, 64, 1)]
VIEWS = [n for n, _ in N.TrainViews._fields_]


def key(shape):
    return "B{}-N{}-d{}-W{}".format(*shape)


def measure(lib, shape):
    batch, n_items, d, window = shape
    ws_bytes = int(lib.cqlrec_train_ws_bytes(batch, n_items, d, window))
    c = N.TrainCtx()
    c.layout = N.make_layout(n_items, d)
    for name in ("offsets", "items", "rewards", "theta", "grads", "adam_m", "adam_v", "target", "theta_b", "target_b"):
        setattr(c, name, 4096)
    c.n_users = 1
    c.batch, c.window, c.world, c.rank = batch, window, 1, 0
    c.ws, c.ws_bytes = WS_BASE, ws_bytes
    steps = []
    for step in STEPS:
        v = N.TrainViews()
        N.check(lib.cqlrec_train_views_get(C.byref(c), step, C.byref(v)), "train_views_get")
        steps.append([int(getattr(v, n)) - WS_BASE for n in VIEWS])
    return {"ws_bytes": ws_bytes, "offsets": steps}


@pytest.fixture(scope="module")
def lib():
    B.build(verbose=False)
    return N.load()


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_golden_file_covers_the_shapes(golden):
    assert golden["views"] == VIEWS and len(VIEWS) == 17
    assert golden["steps"] == list(STEPS)
    assert sorted(golden["shapes"]) == sorted(key(s) for s in SHAPES)


@pytest.mark.parametrize("shape", SHAPES, ids=key)
def test_workspace_size_and_views_are_the_recorded_ones(lib, golden, shape):
    got, want = measure(lib, shape), golden["shapes"][key(shape)]
    assert got["ws_bytes"] == want["ws_bytes"]
    for step, g, w in zip(STEPS, got["offsets"], want["offsets"]):
        assert g == w, (step, [(n, a, b) for n, a, b in zip(VIEWS, g, w) if a != b])


@pytest.mark.parametrize("shape", SHAPES, ids=key)
def test_views_go_by_step_parity(lib, shape):
    o = measure(lib, shape)["offsets"]
    assert o[0] == o[2] and o[1] == o[3]
    assert all(a != b for a, b in zip(o[0], o[1]))      # every view exists twice


if __name__ == "__main__" and "--record" in sys.argv:
    B.build(verbose=False)
    lib_ = N.load()
    GOLDEN.write_text(json.dumps({"views": VIEWS, "steps": list(STEPS),
                                  "shapes": {key(s): measure(lib_, s) for s in SHAPES}}, indent=1) + "\n")
    print(GOLDEN)
