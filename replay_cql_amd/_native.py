"""ctypes binding of libcqlrec.so (the C ABI in include/cqlrec.h).

There is NO fallback: if the HIP library is missing or an entry point is absent, loading raises.  The product path
never routes through oracle/ or any CPU implementation."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Optional

from . import _header
from ._header import CqlrecError, f32, f64, i32, i64, u64, vp  # noqa: F401  (the scalar types, by their short names)

# HIP multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4).  The step driver runs four
# streams concurrently (the caller's + three internal), the predict pass and the data-parallel loop one more each: ask
# for eight -- effective when this module is imported before the first HIP call of the process (importing torch makes
# none); an explicit setting of the user's wins.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

# CQLREC_LIB: another build of the same library (A/B-ing kernel variants with tools/); default: the in-tree build
_LIB_PATH = Path(os.environ["CQLREC_LIB"]).resolve() if os.environ.get("CQLREC_LIB") else \
    Path(__file__).resolve().parent / "libcqlrec.so"
_lib: Optional[C.CDLL] = None

EVAL_EXTRAS = ("RocAuc", "Unexpectedness", "Surprisal", "NCISPrecision")     # names of the header's EVAL_EXTRAS slots


class _LayoutMethods:
    SEGMENTS = ("E_in", "E_out", "b_out", "W1", "b1", "W2", "b2")

    def offset(self, name: str) -> int:
        return int(getattr(self, "off_" + name))

    def shape(self, name: str):
        n, d = int(self.n_items), int(self.d)
        return {"E_in": (n + 1, d), "E_out": (n, d), "b_out": (n,), "W1": (d, d), "b1": (d,), "W2": (d, d),
                "b2": (d,)}[name]


# Everything include/cqlrec.h declares, read from it (_header.py): every `#define CQLREC_X n` as the module attribute X
# (ABI_VERSION and AUX_STREAMS among them), the structs as ctypes Structures, and SIGNATURES = {symbol: (restype,
# argtypes)} -- the table `load` binds and `_device.Engine` reads which arguments are device pointers from.
_H = _header.read(mixins={"Layout": _LayoutMethods})
_K = _H.constants
if _K["EVAL_EXTRAS"] != len(EVAL_EXTRAS):
    raise CqlrecError(f"cqlrec.h has {_K['EVAL_EXTRAS']} extra metrics, _native.EVAL_EXTRAS names {len(EVAL_EXTRAS)}")
globals().update({k: v for k, v in _K.items() if k != "EVAL_EXTRAS"})
Layout, TrainCtx, TrainViews, FeaturesPop = (_H.structs[n] for n in ("Layout", "TrainCtx", "TrainViews", "FeaturesPop"))
SIGNATURES = _H.signatures
PHASES = tuple(k[len("PH_"):].lower() for k in list(_H.enum)[:_H.enum["PH_COUNT"]])
NEIGHBOUR_WEIGHTINGS = {None: _K["NEIGHBOUR_WEIGHT_NONE"], "tf_idf": _K["NEIGHBOUR_WEIGHT_TF_IDF"],
                        "bm25": _K["NEIGHBOUR_WEIGHT_BM25"]}


def prof_read():
    """{phase: (summed kernel ms, launches)} since the last read (synchronises the recorded events)."""
    ms = (C.c_double * len(PHASES))()
    cnt = (i64 * len(PHASES))()
    check(load().cqlrec_prof_read(ms, cnt), "prof_read")
    return {p: (float(ms[i]), int(cnt[i])) for i, p in enumerate(PHASES)}


def lib_path() -> Path:
    return _LIB_PATH


def load() -> C.CDLL:
    """Load the HIP library or raise -- never falls back to anything else."""
    global _lib
    if _lib is not None:
        return _lib
    # torch must be loaded first: it bundles its own libamdhip64, and libcqlrec.so has to bind to that same HIP
    # runtime instance (one runtime per process -- torch's stream handles and device pointers are only valid there).
    import torch  # noqa: F401  pylint: disable=import-outside-toplevel,unused-import
    if not _LIB_PATH.exists():
        raise CqlrecError(
            f"{_LIB_PATH} is missing: build it with `python -m replay_cql_amd.build` (hipcc --offload-arch=gfx950). "
            "replay_cql_amd has no CPU fallback.")
    lib = C.CDLL(str(_LIB_PATH))
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:  # pragma: no cover
            raise CqlrecError(f"{_LIB_PATH} does not export {name}; rebuild it") from exc
        fn.restype, fn.argtypes = res, args
    if lib.cqlrec_abi_version() != _K["ABI_VERSION"]:                # the .so against the header it ships with
        raise CqlrecError(f"libcqlrec ABI {lib.cqlrec_abi_version()} != expected {_K['ABI_VERSION']}; rebuild it")
    _lib = lib
    return lib


_aux_cache: dict = {}


def runtime_init() -> None:
    """Create the library's streams for the CURRENT device now (cqlrec_runtime_init: why the order of stream creation in
    a process decides whether the training step keeps its concurrency).  CQLCore calls this on construction; a
    data-parallel job calls it right after torch.cuda.set_device and BEFORE torch.distributed.init_process_group, whose
    RCCL streams come out of torch's 64-stream pool."""
    check(load().cqlrec_runtime_init(), "runtime_init")


def aux_stream(index: int):
    """Library-owned side stream `index` of the current device as a torch stream object (torch.cuda.ExternalStream):
    side work of the host driver goes there instead of onto a torch.cuda.Stream(), whose first construction creates a
    pool of 64 HIP streams."""
    import torch  # pylint: disable=import-outside-toplevel
    runtime_init()
    dev = torch.cuda.current_device()
    key = (dev, int(index))
    if key not in _aux_cache:
        ptr = load().cqlrec_aux_stream(int(index))
        if not ptr:
            raise CqlrecError(f"no aux stream {index}")
        _aux_cache[key] = torch.cuda.ExternalStream(ptr, device=torch.device("cuda", dev))
    return _aux_cache[key]


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().cqlrec_last_error().decode("utf-8", "replace")
        raise CqlrecError(f"{what or 'cqlrec'} failed (rc={rc}): {msg}")


def make_layout(n_items: int, d: int) -> Layout:
    lay = Layout()
    check(load().cqlrec_layout_make(int(n_items), int(d), C.byref(lay)), "layout_make")
    return lay
