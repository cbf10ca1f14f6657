"""The host layer's known answers: for every public path that drives libcqlrec through the package's Python code, the
sequence of native calls it makes (entry point, every argument rendered by its declared type in `_native.SIGNATURES`:
a pointer as null / non-null, an integer as its value, a float as float.hex, anything else as its ctypes type's name)
and a SHA-256 of what it returns, on one fixed log in each form the API takes (pandas, pyarrow, a dict of device
tensors).  tests/golden/host_calls_known_answers.json holds both as the tree recorded them before the host layer was
given one home, and the scenarios of the rules, ADMMSLIM and SLIM as it recorded them before those
models were given one view builder and one table type per format; these paths are deterministic (sections 3.4-3.10 and
3.13-3.15), so a refactor of the host code must reproduce every trace and every digest.

Only the public API is used, so the file runs unchanged on any checkout:
    python tests/test_gpu_host_calls_known_answers.py --record OUT.json"""
import ctypes as C
import hashlib
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

GOLDEN = ROOT / "tests" / "golden" / "host_calls_known_answers.json"
FORMS = ("pandas", "arrow", "device")
N_USERS, N_ITEMS, HEAVY, HEAVY_ROWS = 40, 30, 3, 1100        # user 17 and item 11 have no row; max ids are present
KS = [1, 5]
ONCE_PER_PROCESS = {"cqlrec_aux_stream"}       # `_native.aux_stream` caches its result: whether it calls depends on what ran before
_INT = (C.c_int32, C.c_int64, C.c_uint64, C.c_uint32)
_FLOAT = (C.c_float, C.c_double)


# ----------------------------------------------------------------------------------------------------------
# the recording proxy and the digest
# ----------------------------------------------------------------------------------------------------------
def _render(ty, v):
    if ty is C.c_void_p:
        return 0 if not (v.value if isinstance(v, C.c_void_p) else v) else 1
    if ty in _INT:
        return int(v.value if hasattr(v, "value") else v)
    if ty in _FLOAT:
        return float(v.value if hasattr(v, "value") else v).hex()
    return ty.__name__


class LibProxy:
    """Stands in for the loaded library: every call is logged, then made."""

    def __init__(self, lib, signatures):
        self._lib, self._sig, self.calls = lib, signatures, []

    def __getattr__(self, name):
        fn, argtypes = getattr(self._lib, name), self._sig[name][1]

        def call(*args):
            assert len(args) == len(argtypes), name
            if name not in ONCE_PER_PROCESS:
                self.calls.append([name] + [_render(ty, v) for ty, v in zip(argtypes, args)])
            return fn(*args)
        return call


def _feed(h, x):
    if x is None or isinstance(x, (bool, int, float, str, np.integer, np.floating)):
        h.update(repr(x).encode())
    elif torch.is_tensor(x):
        _feed(h, x.detach().cpu().contiguous().numpy() if x.dtype != torch.bfloat16 else
              x.detach().cpu().contiguous().view(torch.int16).numpy())
    elif isinstance(x, np.ndarray):
        h.update(f"{x.dtype}{x.shape}".encode())
        h.update(repr(x.tolist()).encode() if x.dtype == object else np.ascontiguousarray(x).tobytes())
    elif isinstance(x, pd.DataFrame):
        for name in x.columns:
            h.update(str(name).encode())
            _feed(h, x[name].to_numpy())
    elif isinstance(x, dict):
        for k, v in x.items():
            h.update(str(k).encode())
            _feed(h, v)
    elif isinstance(x, (list, tuple)):
        h.update(f"seq{len(x)}".encode())
        for v in x:
            _feed(h, v)
    elif hasattr(x, "schema"):                                    # pyarrow Table / RecordBatch
        for name in x.schema.names:
            h.update(str(name).encode())
            col = x.column(name)
            col = col.combine_chunks() if hasattr(col, "combine_chunks") else col
            _feed(h, col.to_numpy(zero_copy_only=False))
    else:
        raise TypeError(f"no digest for {type(x)}")


def digest(x) -> str:
    h = hashlib.sha256()
    _feed(h, x)
    return h.hexdigest()


# ----------------------------------------------------------------------------------------------------------
# the fixed log, in its three forms
# ----------------------------------------------------------------------------------------------------------
def _host_log():
    rng = np.random.default_rng(20261020)
    users = np.array([u for u in range(N_USERS) if u != 17])
    items = np.array([i for i in range(N_ITEMS) if i != 11])
    u = np.concatenate([rng.choice(users, 400), np.full(HEAVY_ROWS, HEAVY), [N_USERS - 1, 0, 5, 5]])
    i = np.concatenate([rng.choice(items, 400 + HEAVY_ROWS), [N_ITEMS - 1, 0, 7, 7]])
    n = len(u)
    order = rng.permutation(n)
    t = 1_600_000_000 + rng.integers(0, 9 * 86400, n)
    r = rng.integers(0, 6, n).astype(np.float64)
    return {"user_idx": u[order].astype(np.int64), "item_idx": i[order].astype(np.int64), "timestamp": t.astype(np.int64),
            "relevance": r}


def as_form(cols, form):
    if form == "pandas":
        return pd.DataFrame(cols)
    if form == "arrow":
        import pyarrow as pa
        return pa.table({k: pa.array(v) for k, v in cols.items()})
    return {k: torch.as_tensor(v).cuda() for k, v in cols.items()}


LOG = _host_log()


def _recs():
    """recommendations (8 per user, distinct items), a ground truth, a base model's lists and a previous policy"""
    rng = np.random.default_rng(7)
    us = np.repeat(np.arange(N_USERS), 8)
    it = np.concatenate([rng.choice(N_ITEMS, 8, replace=False) for _ in range(N_USERS)])
    recs = {"user_idx": us.astype(np.int64), "item_idx": it.astype(np.int64), "relevance": rng.random(len(us))}
    base = {"user_idx": us.astype(np.int64), "item_idx": ((it + 3) % N_ITEMS).astype(np.int64),
            "relevance": rng.random(len(us))}
    prev = {"user_idx": us.astype(np.int64), "item_idx": it.astype(np.int64), "relevance": rng.random(len(us)) + 0.1}
    keep = rng.random(len(LOG["user_idx"])) < 0.2
    gt = {k: v[keep] for k, v in LOG.items()}
    return recs, gt, base, prev


# ----------------------------------------------------------------------------------------------------------
# the scenarios: name -> callable returning what is digested
# ----------------------------------------------------------------------------------------------------------
def scenarios():
    import replay_cql_amd as pkg
    from replay_cql_amd import data as D
    from replay_cql_amd import filters as F
    from replay_cql_amd import history_based_fp as H
    from replay_cql_amd import metrics as M
    from replay_cql_amd import splitters as S
    from replay_cql_amd.admm_slim import ADMMSLIM
    from replay_cql_amd.als import ALSWrap
    from replay_cql_amd.association_rules import AssociationRulesItemRec
    from replay_cql_amd.indexer import Indexer
    from replay_cql_amd.neighbour import ItemKNN
    from replay_cql_amd.slim import SLIM

    out = {}
    log_pd = as_form(LOG, "pandas")

    splitters = {
        "UserSplitter": lambda: S.UserSplitter(item_test_size=2, drop_cold_items=True, drop_zero_rel_in_test=True),
        "DateSplitter": lambda: S.DateSplitter(0.3),
        "RandomSplitter": lambda: S.RandomSplitter(0.25, seed=3),
        "NewUsersSplitter": lambda: S.NewUsersSplitter(0.3),
        "ColdUserRandomSplitter": lambda: S.ColdUserRandomSplitter(0.3, seed=5),
    }
    filters = {
        "filter_by_min_count": lambda lg: F.filter_by_min_count(lg, 10),
        "filter_out_low_ratings": lambda lg: F.filter_out_low_ratings(lg, 2.0),
        "take_num_user_interactions": lambda lg: F.take_num_user_interactions(lg, 3, first=False),
        "take_num_days_of_user_hist": lambda lg: F.take_num_days_of_user_hist(lg, 2),
        "take_time_period": lambda lg: F.take_time_period(lg, "2020-09-15", "2020-09-19"),
        "take_num_days_of_global_hist": lambda lg: F.take_num_days_of_global_hist(lg, 2, first=False),
    }
    raw = {"user_id": LOG["user_idx"] * 7 + 100, "item_id": LOG["item_idx"] * 3 + 5, "relevance": LOG["relevance"]}
    user_features = pd.DataFrame({"user_idx": np.arange(N_USERS), "gender": ["m", "f", None, "f"] * (N_USERS // 4)})
    item_features = pd.DataFrame({"item_idx": np.arange(N_ITEMS), "genre": ["a", "b", "c"] * (N_ITEMS // 3)})
    recs, gt, base, prev = _recs()
    pairs = pd.DataFrame({"user_idx": LOG["user_idx"][:60], "item_idx": (LOG["item_idx"][:60] + 1) % N_ITEMS})
    subset = [0, 2, 4, 6, 8, 10, 12, 29]

    def indexer(form):
        ix = Indexer()
        frame = as_form(raw, form)
        ix.fit(frame, frame)
        fwd = ix.transform(frame)
        return [ix.user_labels, ix.item_labels, fwd, ix.inverse_transform(fwd)]

    def log_stat(form):
        p = H.LogStatFeaturesProcessor()
        p.fit(as_form(LOG, form))
        return p.transform(as_form(LOG, form))

    def cond_pop(form):
        p = H.ConditionalPopularityProcessor(["genre"])
        p.fit(as_form(LOG, form), item_features)
        return p.transform(as_form(LOG, form))

    def history(form):
        p = H.HistoryBasedFeaturesProcessor(user_cat_features_list=["gender"], item_cat_features_list=["genre"])
        p.fit(as_form(LOG, form), user_features, item_features)
        users = torch.as_tensor(LOG["user_idx"][:50]).cuda()
        items = torch.as_tensor(LOG["item_idx"][:50]).cuda()
        return [p.transform(as_form(LOG, form)), p.transform_block(users, items)]

    def metrics(form):
        r, g, lg = as_form(recs, form), as_form(gt, form), as_form(LOG, form)
        res = {}
        for name in ("NDCG", "HitRate", "Precision", "Recall", "MAP", "MRR", "RocAuc"):
            res[name] = getattr(M, name)()(r, g, KS)
        res["NCISPrecision"] = M.NCISPrecision(as_form(prev, form))(r, g, KS)
        res["Surprisal"] = M.Surprisal(lg)(r, KS)
        res["Unexpectedness"] = M.Unexpectedness(as_form(base, form))(r, KS)
        res["Coverage"] = M.Coverage(lg)(r, KS)
        res["item_distribution"] = M.item_distribution(lg, r, 5)
        return res

    def item_knn(form, weighting, **kw):
        m = ItemKNN(num_neighbours=5, weighting=weighting, **kw)
        m.fit(as_form(LOG, form))
        res = [m.similarity_device, m.similarity, m.recommend(as_form(LOG, form), 5),
               m.recommend(as_form(LOG, form), 5, users=[0, 3, 17, 39], items=subset, filter_seen_items=False)]
        if form == "pandas":
            res += [m.predict(log_pd, 5), m.predict(log_pd, 5, filter_seen_items=False), m.predict(log_pd, 5, items=subset),
                    m.predict_pairs(pairs, log_pd), m.get_nearest_items([0, 1, 2, 11], 3)]
        return res

    def item_to_item(m, form, extra, nearest):
        """what every neighbourhood model of the three newer ones is digested by; `extra` names fit's own attributes"""
        m.fit(as_form(LOG, form))
        res = [m.similarity_device, m.similarity, m.recommend(as_form(LOG, form), 5),
               m.recommend(as_form(LOG, form), 5, users=[0, 3, 17, 39], items=subset, filter_seen_items=False)]
        res += [getattr(m, name) for name in extra]
        if form == "pandas":
            res += [m.predict(log_pd, 5), m.predict_pairs(pairs, log_pd), m.get_nearest_items([0, 1, 2, 11], 3, **nearest)]
        return m, res

    def rules(form, **kw):
        m, res = item_to_item(AssociationRulesItemRec(**kw), form, (), {"metric": "confidence_gain"})
        if form == "pandas":
            m.similarity_metric = "confidence"                # the cached CSR has to follow the metric
            res.append(m.predict(log_pd, 5))
        return res

    rules_a = {"num_neighbours": 5}
    rules_b = {"min_item_count": 1, "min_pair_count": 1, "num_neighbours": None, "use_relevance": True,
               "similarity_metric": "lift"}                   # None: k = 29, the all-pairs path

    def admm_slim(form):
        return item_to_item(ADMMSLIM(lambda_1=5, lambda_2=50, seed=7), form, ("rho_sequence", "n_iterations"), {})[1]

    def slim(form):
        return item_to_item(SLIM(beta=50, lambda_=100), form, ("n_sweeps", "kkt", "n_updates", "n_not_converged"), {})[1]

    def als(form, implicit):
        m = ALSWrap(rank=4, implicit_prefs=implicit, seed=1, max_iter=2)
        m.fit(as_form(LOG, form))
        res = [m.factors_device("user"), m.factors_device("item"), m.recommend(as_form(LOG, form), 5),
               m.recommend(None, 5, users=[0, 3, 17, 39], items=subset)]
        if form == "pandas":
            res += [m.predict(log_pd, 5), m.predict(log_pd, 5, filter_seen_items=False, items=subset),
                    m.predict_pairs(pairs), m._get_features_wrap(pd.DataFrame({"user_idx": [0, 17, 39]}), None)[0],
                    m._get_features_wrap(pd.DataFrame({"item_idx": [0, 11, 29]}), None)[0]]
            with tempfile.TemporaryDirectory() as tmp:
                m._save_model(os.path.join(tmp, "als.pt"))
                m2 = ALSWrap()
                m2._load_model(os.path.join(tmp, "als.pt"))
            res += [m2.predict(log_pd, 5), m2.factors_device("item")]
        return res

    def build_csr(form):
        cols = as_form(LOG, "device") if form == "device" else LOG
        full = D.build_csr_device(cols["user_idx"], cols["item_idx"], cols["timestamp"], cols["relevance"], N_USERS)
        seen = D.build_csr_device(cols["user_idx"], cols["item_idx"], None, None, N_USERS)
        return [full, seen]

    def core():
        from replay_cql_amd.core import CQLCore, CQLHyper
        c = CQLCore(N_ITEMS, CQLHyper(d=64, window=8, batch=32, seed=11), device="cuda:0")
        off, items, _ = D.build_csr_device(LOG["user_idx"], LOG["item_idx"], LOG["timestamp"], LOG["relevance"], N_USERS)
        s_off, s_items, _ = D.build_csr_device(LOG["user_idx"], LOG["item_idx"], None, None, N_USERS)
        users = torch.arange(N_USERS, dtype=torch.int32, device="cuda:0")
        hb = c.encode(off, items, users)
        # candidate lists: distinct (user, item) pairs as keys user * N_ITEMS + item, ascending
        key = torch.unique(torch.as_tensor(LOG["user_idx"][:200] * N_ITEMS + (LOG["item_idx"][:200] + 2) % N_ITEMS).cuda())
        bounds = torch.arange(N_USERS + 1, dtype=torch.int64, device="cuda:0") * N_ITEMS
        pair_off = torch.searchsorted(key, bounds).to(torch.int64).contiguous()
        pair_items = (key % N_ITEMS).to(torch.int32).contiguous()
        return [c.item_knn(torch.arange(N_ITEMS), 4, "cosine_similarity"),
                c.pairs_topk(hb, pair_off, pair_items, None, 3, seen=(s_off, s_items)),
                c.score_topk(hb, 5, seen=(s_off, s_items), seen_rows=users),
                c.encode_topk(off, items, users, 5, seen=(s_off, s_items))]

    for form in FORMS:
        for name, make in splitters.items():
            out[f"split.{name}[{form}]"] = lambda make=make, form=form: make().split(as_form(LOG, form))
        out[f"split.k_folds[{form}]"] = lambda form=form: list(S.k_folds(as_form(LOG, form), 2, seed=4))
        for name, fn in filters.items():
            out[f"filter.{name}[{form}]"] = lambda fn=fn, form=form: fn(as_form(LOG, form))
        out[f"indexer[{form}]"] = lambda form=form: indexer(form)
        out[f"features.log_stat[{form}]"] = lambda form=form: log_stat(form)
        out[f"features.cond_pop[{form}]"] = lambda form=form: cond_pop(form)
        out[f"features.history[{form}]"] = lambda form=form: history(form)
        out[f"metrics[{form}]"] = lambda form=form: metrics(form)
        for w in (None, "bm25"):
            out[f"item_knn.{w}[{form}]"] = lambda form=form, w=w: item_knn(form, w)
        for implicit in (True, False):
            out[f"als.{'implicit' if implicit else 'explicit'}[{form}]"] = lambda form=form, i=implicit: als(form, i)
        out[f"rules.a[{form}]"] = lambda form=form: rules(form, **rules_a)
        out[f"rules.b[{form}]"] = lambda form=form: rules(form, **rules_b)
        out[f"admm_slim[{form}]"] = lambda form=form: admm_slim(form)
        out[f"slim[{form}]"] = lambda form=form: slim(form)
    out["item_knn.chunked[device]"] = lambda: item_knn("device", None, max_tuples=500)
    out["rules.chunked[device]"] = lambda: rules("device", max_tuples=500, **rules_a)
    out["build_csr[host]"] = lambda: build_csr("host")
    out["build_csr[device]"] = lambda: build_csr("device")
    out["core"] = core
    assert pkg.__all__
    return out


def run(proxy):
    """{scenario: {"calls": [...], "digest": hex}} -- each scenario's calls are those made while it ran"""
    res = {}
    for name, fn in scenarios().items():
        proxy.calls = []
        value = fn()
        torch.cuda.synchronize()
        res[name] = {"calls": proxy.calls, "digest": digest(value)}
    return res


def _proxy():
    from replay_cql_amd import _native as N
    return N, LibProxy(N.load(), N.SIGNATURES)


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.fixture(scope="module")
def recorded():
    N, proxy = _proxy()
    mp = pytest.MonkeyPatch()
    mp.setattr(N, "_lib", proxy)
    try:
        return run(proxy)
    finally:
        mp.undo()


@pytest.mark.gpu
def test_every_scenario_was_recorded(golden, recorded):
    assert sorted(golden) == sorted(recorded)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["calls", "digest"])
def test_host_calls_and_results_are_the_recorded_ones(golden, recorded, what):
    differ = [name for name in golden if what in golden[name] and golden[name][what] != recorded[name][what]]
    for name in differ[:3]:
        if what == "calls":
            a, b = golden[name]["calls"], recorded[name]["calls"]
            at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print(f"{name}: call {at} of {len(a)} / {len(b)}: recorded {a[at:at + 1]}, now {b[at:at + 1]}")
    assert not differ, f"{what} differ from the recorded ones in {len(differ)} scenarios: {differ}"
    assert all("calls" in golden[name] for name in golden)


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    native, prox = _proxy()
    native._lib = prox
    Path(sys.argv[2]).write_text(json.dumps(run(prox), separators=(",", ":"), sort_keys=True))
    print(f"recorded {sys.argv[2]}")
