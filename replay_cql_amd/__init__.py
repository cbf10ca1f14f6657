"""replay_cql_amd -- MI355X-native CQL recommender hot path behind the RePlay Recommender API.

Only what the path needs: csrc/ (HIP kernels + C ABI, built into libcqlrec.so), _native (ctypes binding),
core (device driver).  The HIP library is loaded lazily; nothing here falls back to a CPU implementation."""
__version__ = "0.1.0"

# the train/test splitters (splitters.py), importable from the package without loading torch until they are asked for
_SPLITTERS = ("Splitter", "UserSplitter", "DateSplitter", "RandomSplitter", "NewUsersSplitter", "ColdUserRandomSplitter",
              "k_folds")
__all__ = list(_SPLITTERS)


def __getattr__(name):
    if name in _SPLITTERS:
        from . import splitters          # pylint: disable=import-outside-toplevel
        return getattr(splitters, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
