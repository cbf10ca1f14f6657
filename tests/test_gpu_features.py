"""The history-based feature processors on the GPU (replay_cql_amd.history_based_fp, csrc/features.hip) against the known
answers of tests/golden/history_features_known_answers.json and the numpy yardstick tests/features_reference.py.

Equality rules.  Exact: counts, distinct days, dates, both day differences, all quantiles, the `na` flags, the column
sets and their order; `mean` on the dyadic logs (the sums are exact in fp64 in any order, one division is left).
Every other float: |got - ref| <= 8 * n_g * 2^-53 * max(|ref|, s_g), n_g the group's row count and s_g the largest
magnitude entering the statistic in the group (features_reference.tolerance has the derivation)."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest
import torch

import features_reference as R
from replay_cql_amd import history_based_fp as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = R.golden()
EXACT = ("quantile_05", "quantile_5", "quantile_95", "history_length_days", "last_interaction_gap_days", "mean")
_CACHE = {}


def build_log(name):
    """(log dict of numpy columns, its yardstick fit), computed once"""
    if name not in _CACHE:
        kind, _, ts = name.partition("/")
        if kind == "sizes":
            log = R.sizes_log()[0]
        else:
            log = R.ties_log(2.0 ** 20 if kind == "offset" else 0.0)
        if ts == "datetime":
            log = R.as_datetime(log)
        _CACHE[name] = (log, R.fit_reference(log))
    return _CACHE[name]


def given(log):
    """datetime64 has no torch dtype: those logs go in as pandas, the others as device tensors"""
    if log["timestamp"].dtype.kind == "M":
        return pd.DataFrame(log)
    return {k: torch.as_tensor(v).to(DEV) for k, v in log.items()}


def fitted(name):
    if ("fit", name) not in _CACHE:
        proc = H.LogStatFeaturesProcessor()
        proc.fit(given(build_log(name)[0]))
        _CACHE["fit", name] = proc
    return _CACHE["fit", name]


def check_tables(proc, ref, what):
    """every fitted table of `proc` against the yardstick fit `ref`, by the module's equality rules"""
    assert proc.calc_relevance_based == ref["calc_relevance_based"], what
    assert proc.calc_timestamp_based == ref["calc_timestamp_based"], what
    worst = {}
    for pre, tab, names, count, dates, days in (("u", proc._utab, proc._unames, proc._ucount, proc._udates, proc._udays),
                                                ("i", proc._itab, proc._inames, proc._icount, proc._idates, proc._idays)):
        side = ref[pre]
        assert names == R.feature_names(ref, pre, dates=False), (what, names)
        assert np.array_equal(count.cpu().numpy(), side["count"]), (what, pre, "count")
        present = side["count"] > 0
        tab = tab.cpu().numpy()
        assert tab.shape == (len(side["count"]), len(names)) and not tab[~present].any(), (what, pre, "cold rows")
        if ref["calc_timestamp_based"]:
            assert np.array_equal(days.cpu().numpy(), side["cols"][pre + "_distinct_days"]), (what, pre, "days")
            for which, keys in zip(("min", "max"), dates):
                want = side["cols"][f"{pre}_{which}_interact_date"]
                assert np.array_equal(keys.cpu().numpy()[present], want[present]), (what, pre, which)
        for j, name in enumerate(names):
            want, got = side["cols"][name].astype(np.float64), tab[:, j]
            if name[2:] in EXACT:
                assert np.array_equal(got, want), (what, name, np.flatnonzero(got != want)[:5])
                continue
            tol = R.tolerance(ref, pre, name)
            err = np.abs(got - want)
            k = int(np.argmax(err - tol))
            worst[name] = float(np.max(err / np.maximum(tol, 1e-300)))
            print(f"{what} {name}: worst |err| / tolerance = {worst[name]:.3g} (id {k}: got {got[k]!r} ref {want[k]!r} "
                  f"n_g {side['count'][k]})")
            assert (err <= tol).all(), (what, name, k, got[k], want[k], tol[k])
    return worst


def frame_of(case):
    return pd.DataFrame(R.golden_log(GOLDEN, case))


# ---------------------------------------------------------------------------------------------------------------------
# the known answers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["no_ts_rel", "ts_no_rel", "relevance_ts"])
def test_known_answers(case):
    groups, want = GOLDEN["column_groups"], GOLDEN["cases"][case]
    proc = H.LogStatFeaturesProcessor()
    proc.fit(frame_of(case))
    u_cols, i_cols = ["user_idx"] + groups["simple_u"], ["item_idx"] + groups["simple_i"]
    if case != "no_ts_rel":
        u_cols += ["u_" + c for c in groups["time"]]
        i_cols += ["i_" + c for c in groups["time"]]
    if case == "relevance_ts":
        u_cols += ["u_" + c for c in groups["relevance"]] + groups["abnormality"]
        i_cols += ["i_" + c for c in groups["relevance"]]
    users, items = proc.user_log_features, proc.item_log_features
    assert sorted(users.columns) == sorted(u_cols) and sorted(items.columns) == sorted(i_cols)
    assert users["user_idx"].tolist() == [0, 1, 2] and items["item_idx"].tolist() == [0, 1, 2, 3]
    for frame, side in ((users, "user"), (items, "item")):
        if side + "_columns" not in want:
            continue
        for row in want[side + "_rows"]:
            got = frame[frame[side + "_idx"] == GOLDEN["ids"][side][row[0]]].iloc[0]
            for name, value in zip(want[side + "_columns"][1:], row[1:]):
                if name.endswith("_interact_date"):
                    assert got[name] == pd.Timestamp(value), (name, row)
                elif isinstance(value, int) or "quantile" in name:
                    assert got[name] == value, (name, row)
                else:
                    assert abs(got[name] - value) <= 1e-12, (name, row, got[name])
    check_tables(proc, R.fit_reference(R.golden_log(GOLDEN, case)), case)


def feature_frames():
    ids = GOLDEN["ids"]
    users = pd.DataFrame([[ids["user"][r[0]]] + r[1:] for r in GOLDEN["user_features"]["rows"]],
                         columns=GOLDEN["user_features"]["columns"])
    items = pd.DataFrame([[ids["item"][r[0]]] + r[1:] for r in GOLDEN["item_features"]["rows"]],
                         columns=GOLDEN["item_features"]["columns"])
    return users, items


def test_conditional_popularity_known_answers():
    users, _ = feature_frames()
    proc = H.ConditionalPopularityProcessor(cat_features_list=["gender"])
    proc.fit(log=frame_of("relevance_ts"), features=users)
    assert proc.entity_name == "item_idx"
    got = proc.conditional_pop_dict["gender"]
    assert list(got.columns) == GOLDEN["cases"]["conditional_features"]["columns"]
    got = got[got["item_idx"].isin([0, 1])]
    rows = {(int(r.item_idx), r.gender): r.i_pop_by_gender for r in got.itertuples()}
    assert rows == {(GOLDEN["ids"]["item"][r[0]], r[1]): r[2] for r in GOLDEN["cases"]["conditional_features"]["rows"]}
    with pytest.raises(ValueError, match="defined in `cat_features_list` are absent in features"):
        H.ConditionalPopularityProcessor(["age"]).fit(frame_of("relevance_ts"), users)


def test_history_based_fp_fit_transform():
    users, items = feature_frames()
    fp = H.HistoryBasedFeaturesProcessor(user_cat_features_list=["gender"], item_cat_features_list=["class"])
    log = frame_of("relevance_ts")
    with pytest.raises(AttributeError, match="Call fit before running transform"):
        fp.transform(log)
    fp.fit(log, users, items)
    assert fp.fitted and fp.log_processor.user_log_features is not None
    assert "i_pop_by_gender" in fp.user_cond_pop_proc.conditional_pop_dict["gender"].columns
    joined = log.merge(users, on="user_idx").merge(items, on="item_idx")
    res = fp.transform(joined)
    assert isinstance(res, pd.DataFrame) and len(res) == len(joined)
    assert list(res.columns[:len(joined.columns)]) == list(joined.columns)
    for name in GOLDEN["cases"]["fit_transform"]["expect_columns"] + ["u_pop_by_class", "na_i_pop_by_gender"]:
        assert name in res.columns
    assert res["na_u_pop_by_class"].dtype == bool and not res["na_u_pop_by_class"].any()
    # i1 (item 0) was seen once by a man and once by a woman; u1 (user 0) saw two cats
    first = res[(res["user_idx"] == 0) & (res["item_idx"] == 0)].iloc[0]
    assert first["i_pop_by_gender"] == 0.5 and first["u_pop_by_class"] == 1.0 and first["na_u_log_features"] == 0.0


def test_history_based_fp_one_features_df():
    users, _ = feature_frames()
    fp = H.HistoryBasedFeaturesProcessor(user_cat_features_list=["gender"])
    fp.fit(log=frame_of("relevance_ts"), user_features=users)
    assert type(fp.item_cond_pop_proc) is H.EmptyFeatureProcessor
    assert "i_pop_by_gender" in fp.user_cond_pop_proc.conditional_pop_dict["gender"].columns
    res = fp.transform(frame_of("relevance_ts").merge(users, on="user_idx"))
    assert "i_pop_by_gender" in res.columns
    # the deviation: an item list alone builds the item-side processor
    only_items = H.HistoryBasedFeaturesProcessor(item_cat_features_list=["class"])
    assert isinstance(only_items.item_cond_pop_proc, H.ConditionalPopularityProcessor)
    assert type(only_items.user_cond_pop_proc) is H.EmptyFeatureProcessor


# ---------------------------------------------------------------------------------------------------------------------
# against the yardstick
# ---------------------------------------------------------------------------------------------------------------------
def test_one_row():
    log = {"user_idx": np.array([2]), "item_idx": np.array([1]), "timestamp": np.array([5]), "relevance": np.array([3.0])}
    proc = H.LogStatFeaturesProcessor()
    proc.fit(given(log))
    check_tables(proc, R.fit_reference(log), "one row")
    assert proc._unames == ["u_log_num_interact", "u_mean_i_log_num_interact"] and proc._utab.shape == (3, 2)
    assert proc.user_log_features["user_idx"].tolist() == [2] and not proc._utab.any()
    block, names = proc.transform_block(torch.tensor([2, 0], device=DEV), torch.tensor([1, 1], device=DEV), torch.float64)
    assert names == R.block_names(R.fit_reference(log))
    assert block.cpu().tolist() == [[0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0, 0]]


@pytest.mark.parametrize("name", ["ties/int", "ties/datetime", "offset/int", "sizes/int"])
def test_fit_against_the_yardstick(name):
    log, ref = build_log(name)
    assert ref["calc_relevance_based"] and ref["calc_timestamp_based"] and ref["has_cr"]
    proc = fitted(name)
    check_tables(proc, ref, name)
    users = proc.user_log_features
    assert list(users.columns) == ["user_idx"] + R.feature_names(ref, "u")
    assert users["user_idx"].tolist() == np.flatnonzero(ref["u"]["count"]).tolist()
    assert users["u_history_length_days"].dtype == np.int64
    if name.endswith("datetime"):
        assert users["u_min_interact_date"].dtype == np.dtype("datetime64[ns]")
        assert np.array_equal(users["u_max_interact_date"].to_numpy().astype(np.int64),
                              ref["u"]["cols"]["u_max_interact_date"][ref["u"]["count"] > 0])


def test_a_float_timestamp_column_gives_no_time_features():
    log = dict(build_log("ties/int")[0])
    log["timestamp"] = log["timestamp"].astype(np.float64)
    proc = H.LogStatFeaturesProcessor()
    proc.fit(given(log))
    assert proc.calc_relevance_based and not proc.calc_timestamp_based
    check_tables(proc, R.fit_reference(log), "float timestamps")
    with pytest.raises(ValueError, match="NaN"):
        H.LogStatFeaturesProcessor().fit(given(dict(log, relevance=np.where(log["item_idx"] == 3, np.nan, 1.0))))


def tables(proc):
    return [proc._utab, proc._itab, proc._ucount, proc._icount, proc._udays, proc._idays, *proc._udates, *proc._idates]


def test_two_fits_give_the_same_bytes_and_a_shuffled_log_agrees():
    log, ref = build_log("offset/int")
    first = fitted("offset/int")
    again = H.LogStatFeaturesProcessor()
    again.fit(given(log))
    for a, b in zip(tables(first), tables(again)):
        assert torch.equal(a, b) and a.dtype == b.dtype
    order = np.random.default_rng(3).permutation(len(log["user_idx"]))
    shuffled = H.LogStatFeaturesProcessor()
    shuffled.fit(given({k: v[order] for k, v in log.items()}))
    check_tables(shuffled, ref, "shuffled")               # exact columns exactly, the others within the tolerance


def test_an_empty_log_fits_to_empty_tables():
    empty = {k: torch.as_tensor(v[:0]).to(DEV) for k, v in build_log("ties/int")[0].items()}
    proc = H.LogStatFeaturesProcessor()
    proc.fit(empty)
    assert proc._utab.shape == (0, 2) and proc._itab.shape == (0, 2) and len(proc.user_log_features) == 0
    block, names = proc.transform_block(torch.tensor([0, 5], device=DEV), torch.tensor([1, 0], device=DEV))
    assert block.dtype == torch.float32 and block.cpu().tolist() == [[0, 0, 0, 0, 1, 1, 0, 0]] * 2
    pop = H.ConditionalPopularityProcessor(["c"])
    pop.fit(empty, pd.DataFrame({"user_idx": [0, 1], "c": ["a", "b"]}))
    assert len(pop.conditional_pop_dict["c"]) == 0


# ---------------------------------------------------------------------------------------------------------------------
# conditional popularity, transform and transform_block
# ---------------------------------------------------------------------------------------------------------------------
def categories(log):
    """user -> age group (strings, None for some, a fifth of the users missing), item -> class (floats with NaN)"""
    rng = np.random.default_rng(5)
    users = np.unique(log["user_idx"])
    users = users[rng.random(len(users)) > 0.2]
    age = rng.choice(np.array(["young", "adult", "old", None], dtype=object), len(users))
    items = np.unique(log["item_idx"])[::2]
    cls = rng.choice([1.5, 2.5, np.nan], len(items))
    return (pd.DataFrame({"user_idx": users, "age": age, "noise": rng.random(len(users))}),
            pd.DataFrame({"item_idx": items, "class": cls}))


def full_processor():
    if "full" not in _CACHE:
        log = build_log("ties/int")[0]
        users, items = categories(log)
        fp = H.HistoryBasedFeaturesProcessor(user_cat_features_list=["age"], item_cat_features_list=["class"])
        fp.fit(given(log), users, items)
        _CACHE["full"] = (fp, users, items)
    return _CACHE["full"]


def test_conditional_popularity_against_the_yardstick():
    log = build_log("ties/int")[0]
    fp, users, items = full_processor()
    for proc, feats, col, entity, other in ((fp.user_cond_pop_proc, users, "age", "item_idx", "user_idx"),
                                            (fp.item_cond_pop_proc, items, "class", "user_idx", "item_idx")):
        want = R.conditional_popularity(log[entity], log[other], dict(zip(feats[other].tolist(), feats[col].tolist())))
        got = proc.conditional_pop_dict[col]
        assert list(got.columns) == [entity, col, f"{entity[0]}_pop_by_{col}"]
        got = {(int(e), None if c is None else c): p for e, c, p in got.itertuples(index=False)}
        assert len(got) == len(want) and any(c is None for _, c in got)
        assert got == {(e, c): p for e, c, p in want}       # counts are integers and the share is one division: exact


def pairs(n, log):
    """n pairs: known ids, cold ids inside the tables, ids beyond them and a negative one"""
    rng = np.random.default_rng(n)
    user = rng.integers(0, 330, n)
    item = rng.integers(0, 110, n)
    user[0], item[0] = log["user_idx"][0], log["item_idx"][0]
    if n > 2:
        user[1], item[2] = -1, 5000
    return user.astype(np.int64), item.astype(np.int64)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 10007])
def test_transform_block_and_transform(n):
    log, ref = build_log("ties/int")
    fp, users, items = full_processor()
    user, item = pairs(n, log)
    du, di = torch.as_tensor(user).to(DEV), torch.as_tensor(item).to(DEV)
    block, names = fp.transform_block(du, di, torch.float64)
    pop_names = ["i_pop_by_age", "na_i_pop_by_age", "u_pop_by_class", "na_u_pop_by_class"]
    assert names == R.block_names(ref) + pop_names
    assert block.shape == (n, len(names)) and block.dtype == torch.float64 and block.is_contiguous()
    b32, names32 = fp.transform_block(du, di)
    assert names32 == names and b32.dtype == torch.float32 and torch.equal(b32, block.to(torch.float32))
    got = dict(zip(names, block.cpu().numpy().T))
    # the log features: the yardstick's left join over the FITTED tables (checked against the yardstick's in the fit tests)
    proc = fp.log_processor
    fit_tables = {pre: {"count": c.cpu().numpy(), "cols": dict(zip(nm, t.cpu().numpy().T))}
                  for pre, c, nm, t in (("u", proc._ucount, proc._unames, proc._utab),
                                        ("i", proc._icount, proc._inames, proc._itab))}
    want = R.transform(fit_tables, user, item)
    for name in R.block_names(ref):
        assert np.array_equal(got[name], want[name]), name
    assert got["na_u_log_features"][0] == 0 and (n < 3 or (got["na_u_log_features"][1] == 1 and got["na_i_log_features"][2] == 1))
    # the popularity columns, the category coming from the table fitted per id
    for col, feats, entity, other, e_ids, o_ids in (("age", users, "item_idx", "user_idx", item, user),
                                                    ("class", items, "user_idx", "item_idx", user, item)):
        lookup = dict(zip(feats[other].tolist(), feats[col].tolist()))
        table = R.conditional_popularity(log[entity], log[other], lookup)
        cats = [lookup.get(int(o)) for o in o_ids]
        cats = [None if c is None or c != c else c for c in cats]
        share, na = R.popularity_lookup(table, e_ids, cats)
        e = entity[0]
        assert np.array_equal(got[f"{e}_pop_by_{col}"], share), col
        assert np.array_equal(got[f"na_{e}_pop_by_{col}"], na.astype(np.float64)), col
    # the frame path: the same columns bit for bit, every kind back as it came, rows in input order
    frame = pd.DataFrame({"user_idx": user, "item_idx": item, "score": np.arange(n, dtype=np.float64)})
    for kind in ("pandas", "arrow", "batch", "tensors"):
        src = {"pandas": frame, "arrow": pa.Table.from_pandas(frame, preserve_index=False),
               "batch": pa.RecordBatch.from_pandas(frame, preserve_index=False),
               "tensors": {k: torch.as_tensor(frame[k].to_numpy()).to(DEV) for k in frame.columns}}[kind]
        res = fp.transform(src)
        if kind == "tensors":
            assert isinstance(res, dict) and all(v.is_cuda for v in res.values())
            res = pd.DataFrame({k: v.cpu().numpy() for k, v in res.items()})
        else:
            assert isinstance(res, type(src))
            res = res if kind == "pandas" else res.to_pandas()
        assert list(res.columns[:3]) == ["user_idx", "item_idx", "score"] and res["score"].tolist() == frame["score"].tolist()
        assert [c for c in res.columns[3:] if not c.endswith("_interact_date")] == names
        assert sum(c.endswith("_interact_date") for c in res.columns) == 4
        for name in names:
            col = res[name].to_numpy()
            if name.startswith("na_") and "_pop_by_" in name:
                assert col.dtype == bool
            assert np.array_equal(col.astype(np.float64), got[name]), (kind, name)
        cold = got["na_u_log_features"] == 1
        dates = res["u_max_interact_date"]
        if kind == "tensors":
            assert (dates.to_numpy()[cold] == np.iinfo(np.int64).min).all()
        else:
            assert dates.isna().to_numpy().tolist() == cold.tolist()
        known = dates.to_numpy()[~cold].astype(np.int64)
        assert np.array_equal(known, ref["u"]["cols"]["u_max_interact_date"][user[~cold]])


def test_the_frames_own_category_column_wins_and_unseen_or_null_values_are_na():
    log = build_log("ties/int")[0]
    fp, users, _ = full_processor()
    proc = fp.user_cond_pop_proc
    table = R.conditional_popularity(log["item_idx"], log["user_idx"], dict(zip(users["user_idx"].tolist(), users["age"].tolist())))
    item = np.array([0, 0, 0, 0, 1, 96, 5000], dtype=np.int64)
    age = np.array(["young", "old", "ancient", None, "adult", "young", "young"], dtype=object)
    frame = pd.DataFrame({"user_idx": np.zeros(7, dtype=np.int64), "item_idx": item, "age": age})
    res = proc.transform(frame)
    share, na = R.popularity_lookup(table, item, age.tolist())
    assert list(res.columns) == ["user_idx", "item_idx", "age", "i_pop_by_age", "na_i_pop_by_age"]
    assert np.array_equal(res["i_pop_by_age"].to_numpy(), share) and res["na_i_pop_by_age"].tolist() == na.tolist()
    assert na.tolist()[2:4] == [True, True] and not na[0] and na[6]
