"""The one home of a call into libcqlrec from Python: `Engine`, the base of every class that
drives a section of include/cqlrec.h on one device, and `_ptr`."""
from __future__ import annotations

import torch

from . import _native as N


def _ptr(t):
    return None if t is None else t.data_ptr()


class Ws:
    """In `Engine.call`, stands where the entry point takes its (ws, ws_bytes) pair; holds the size arguments of the
    matching `*_ws_bytes` query."""

    def __init__(self, *sizes):
        self.sizes = sizes


_PLANS = {}


def _plan(name: str, args):
    """(the entry point's symbol, the positions in `args` that hold pointers, the position of the `Ws` or None), made
    once per entry point from its argument types in `_native.SIGNATURES`, i.e. from its prototype in include/cqlrec.h"""
    types = list(N.SIGNATURES["cqlrec_" + name][1][:-1])                   # the stream is appended by `call`
    ws_at = next((i for i, a in enumerate(args) if isinstance(a, Ws)), None)
    if ws_at is not None:
        del types[ws_at + 1]                                              # the marker stands for (ws, ws_bytes)
    if len(types) != len(args):
        raise TypeError(f"cqlrec_{name} takes {len(types)} arguments before the stream, not {len(args)}")
    ptrs = tuple(i for i, t in enumerate(types) if t is N.vp and i != ws_at)
    _PLANS[name] = plan = ("cqlrec_" + name, ptrs, ws_at)
    return plan


class Engine:
    """The calls into libcqlrec on one device, on the stream OF THAT DEVICE (not of the current one); a device that is
    no GPU is refused here, by torch, before a host pointer can reach a kernel."""

    def __init__(self, device):
        self.N, self.lib, self.dev = N, N.load(), device
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream

    def _empty(self, n, dt):
        return torch.empty(int(n), dtype=dt, device=self.dev)

    def _ws(self, nbytes: int):
        return self._empty(nbytes, torch.uint8)

    def ws_bytes(self, name: str, *sizes) -> int:
        """cqlrec_<name>_ws_bytes(*sizes), for a call site that must see the size or bring its own workspace"""
        return int(getattr(self.lib, f"cqlrec_{name}_ws_bytes")(*sizes))

    def call(self, name: str, *args) -> None:
        """cqlrec_<name>(*args, stream), the arguments in header order: at a pointer position a tensor (a host tensor too)
        goes as its data_ptr() and None as a null pointer; numbers and ctypes objects go as they are; a `Ws` is queried,
        allocated and spliced in as (pointer, bytes) and lives until the call is enqueued.  A non-zero return raises
        CqlrecError."""
        symbol, ptrs, ws_at = _PLANS.get(name) or _plan(name, args)
        flat = list(args)
        for i in ptrs:
            if flat[i] is not None:
                flat[i] = flat[i].data_ptr()
        if ws_at is not None:
            nb = self.ws_bytes(name, *flat[ws_at].sizes)
            ws = self._ws(nb)
            flat[ws_at:ws_at + 1] = [ws.data_ptr(), nb]
        N.check(getattr(self.lib, symbol)(*flat, self.stream), name)
