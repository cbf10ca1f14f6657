"""`_device.Engine.call` marshals its arguments on the host: checked on CPU tensors against a
stand-in for the library, and through the real library where an entry point rejects its arguments before any HIP call.
No GPU: the engine of these tests is given a host device and a null stream in place of torch's."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

from replay_cql_amd import _native as N
from replay_cql_amd._device import Engine, Ws, _ptr


class FakeLib:
    """records what reaches the entry points; a 64-byte workspace per size argument"""

    def __init__(self):
        self.seen = []

    def cqlrec_prepare_rank_ws_bytes(self, *sizes):
        self.seen.append(("ws_bytes", sizes))
        return 64 * len(sizes)

    def cqlrec_prepare_rank(self, *args):
        self.seen.append(("call", args))
        return 0


@pytest.fixture
def host_engine(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device: SimpleNamespace(cuda_stream=None))
    return Engine("cpu")


def test_an_engine_is_refused_a_host_device():
    with pytest.raises((ValueError, RuntimeError)):       # torch's "Expected a cuda device", or its "No HIP GPUs" without one
        Engine("cpu")


def test_ptr():
    t = torch.zeros(3)
    assert _ptr(None) is None and _ptr(t) == t.data_ptr()


def test_call_marshals_tensors_none_numbers_and_the_workspace(host_engine):
    eng = host_engine
    eng.lib = fake = FakeLib()
    assert eng.stream is None
    t = torch.arange(5, dtype=torch.int64)
    eng.call("prepare_rank", t, t[2:], None, 5, 7, 0, Ws(1000, 10), t, None)        # the header's order, the stream left out
    (kind, sizes), (_, args) = fake.seen
    assert kind == "ws_bytes" and sizes == (1000, 10)
    assert args[:6] == (t.data_ptr(), t.data_ptr() + 16, None, 5, 7, 0)
    assert isinstance(args[6], int) and args[6] != 0 and args[7] == 128          # the (pointer, bytes) pair, spliced in place
    assert args[8:] == (t.data_ptr(), None, None) and len(args) == 11            # the stream comes last


def test_numbers_and_ctypes_objects_pass_through(host_engine):
    eng = host_engine
    got = []
    eng.lib = SimpleNamespace(cqlrec_eval_coverage=lambda *args: got.extend(args) or 0)
    t, ks = torch.zeros(4, dtype=torch.int32), (C.c_int32 * 2)(1, 5)
    eng.call("eval_coverage", t, t, 2, 2, 30, ks, 2, t, None)
    assert got[2:5] == [2, 2, 30] and got[5] is ks and got[6] == 2 and got[0] == got[7] == t.data_ptr() and got[8] is None


def test_a_wrong_argument_count_is_refused_before_the_call(host_engine):
    with pytest.raises(TypeError, match="cqlrec_prepare_minmax takes 6 arguments"):
        host_engine.call("prepare_minmax", None, None, 10)


def test_workspace_marker_takes_the_size_the_library_gives(host_engine):
    eng = host_engine
    want = int(N.load().cqlrec_prepare_rank_ws_bytes(1000, 10))
    assert want > 0 and eng.ws_bytes("prepare_rank", 1000, 10) == want
    real, got = eng.lib, []

    class Spy:
        cqlrec_prepare_rank_ws_bytes = staticmethod(real.cqlrec_prepare_rank_ws_bytes)

        @staticmethod
        def cqlrec_prepare_rank(*args):
            got.extend(args)
            return 0

    eng.lib = Spy
    eng.call("prepare_rank", None, None, None, 1000, 10, 0, Ws(1000, 10), None, None)
    assert got[7] == want and got[6] != 0 and len(got) == 11


def test_a_rejected_call_raises_with_the_entry_points_name(host_engine):
    eng = host_engine
    with pytest.raises(N.CqlrecError, match=r"^prepare_count failed \(rc="):
        eng.call("prepare_count", None, -1, 10, None)
