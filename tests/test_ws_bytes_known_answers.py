"""Every *_ws_bytes query of the files on csrc/segment_common.h (prep, metrics, split, prepare, features, neighbour, als,
gbwd) returns exactly what it returned before those files shared their size formulas: callers size allocations from these
numbers and the entry points carve their workspaces by the same formulas.  tests/golden/ws_bytes_known_answers.json was
recorded from the build of the commit BEFORE the shared header, per size argument over -1, 0, 1, 255, 256, 257, 100 003 and
2^31 - 1 (crossed sparingly where a function has several), with two legal values for rank / d / k / n_ks / L.  The queries
are host-only: no GPU is needed."""
import json
from pathlib import Path

import pytest

from replay_cql_amd import _native as N
from replay_cql_amd import build as B

RECORDS = json.loads((Path(__file__).resolve().parent / "golden" / "ws_bytes_known_answers.json").read_text())
FUNCTIONS = sorted({r[0] for r in RECORDS})


@pytest.fixture(scope="module")
def lib():
    B.build(verbose=False)
    return N.load()


def test_the_grid_is_complete():
    grid = {-1, 0, 1, 255, 256, 257, 100003, 2 ** 31 - 1}
    assert len(FUNCTIONS) == 25 and len(RECORDS) >= 600
    for fn in FUNCTIONS:
        firsts = {r[1][0] for r in RECORDS if r[0] == fn}
        assert grid <= firsts, fn


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_ws_bytes_is_what_it_was(lib, fn):
    f = getattr(lib, fn)
    bad = [(args, want, int(f(*args))) for name, args, want in RECORDS if name == fn and int(f(*args)) != want]
    assert not bad, bad[:5]
