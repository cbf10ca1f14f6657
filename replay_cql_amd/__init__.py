"""replay_cql_amd -- MI355X-native CQL recommender hot path behind the RePlay Recommender API.

Only what the path needs: csrc/ (HIP kernels + C ABI, built into libcqlrec.so), _native (ctypes binding),
core (device driver).  The HIP library is loaded lazily; nothing here falls back to a CPU implementation."""
__version__ = "0.1.0"

# the train/test splitters (splitters.py), the filters (filters.py), the Indexer (indexer.py) and the history-based
# feature processors (history_based_fp.py), the neighbourhood models (neighbour.py), association rules
# (association_rules.py), ALS (als.py), ADMM SLIM (admm_slim.py) and SLIM (slim.py), importable from the package without loading torch until they are asked for
_SPLITTERS = ("Splitter", "UserSplitter", "DateSplitter", "RandomSplitter", "NewUsersSplitter", "ColdUserRandomSplitter",
              "k_folds")
_FILTERS = ("filter_by_min_count", "filter_out_low_ratings", "take_num_user_interactions", "take_num_days_of_user_hist",
            "take_time_period", "take_num_days_of_global_hist")
_FEATURES = ("EmptyFeatureProcessor", "LogStatFeaturesProcessor", "ConditionalPopularityProcessor",
             "HistoryBasedFeaturesProcessor")
_NEIGHBOUR = ("NeighbourRec", "ItemKNN")
__all__ = list(_SPLITTERS) + list(_FILTERS) + ["Indexer"] + list(_FEATURES) + list(_NEIGHBOUR) + ["ALSWrap", "AssociationRulesItemRec", "ADMMSLIM", "SLIM"]


def __getattr__(name):
    if name in _SPLITTERS:
        from . import splitters          # pylint: disable=import-outside-toplevel
        return getattr(splitters, name)
    if name in _FILTERS:
        from . import filters            # pylint: disable=import-outside-toplevel
        return getattr(filters, name)
    if name in _FEATURES:
        from . import history_based_fp   # pylint: disable=import-outside-toplevel
        return getattr(history_based_fp, name)
    if name in _NEIGHBOUR:
        from . import neighbour          # pylint: disable=import-outside-toplevel
        return getattr(neighbour, name)
    if name == "AssociationRulesItemRec":
        from . import association_rules  # pylint: disable=import-outside-toplevel
        return association_rules.AssociationRulesItemRec
    if name == "ADMMSLIM":
        from . import admm_slim          # pylint: disable=import-outside-toplevel
        return admm_slim.ADMMSLIM
    if name == "SLIM":
        from . import slim               # pylint: disable=import-outside-toplevel
        return slim.SLIM
    if name == "ALSWrap":
        from . import als                # pylint: disable=import-outside-toplevel
        return als.ALSWrap
    if name == "Indexer":
        from . import indexer            # pylint: disable=import-outside-toplevel
        return indexer.Indexer
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
