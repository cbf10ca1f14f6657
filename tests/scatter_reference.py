"""Float64 references and DERIVED element bounds for the step's scatter and state-side kernels, the crafted key layouts
of the segmented-sum tests, and a NumPy port of the two-pass segmented sum (gbwd.hip).  NumPy only: the CPU self-test
(test_scatter_reference_cpu.py) and the GPU modules (test_gpu_scatter_rows.py, test_gpu_state_side_rows.py) share it.

The bound.  A sum of n fp32 terms accumulated in fp32 IN ANY ORDER, each term carrying at most two roundings of its own
(the product, and the division or weight), satisfies

    |got - ref64| <= (n + 2) u sum_i |t_i|,      u = 2^-24,

with ref64 and sum |t_i| formed in float64 from the kernel's own inputs (n - 1 additions and two roundings per term: to
first order (n + 1) u; the remaining u covers the higher-order terms, n u << 1 everywhere here).  The relative bound
holds for normal fp32 results; an operation whose result is subnormal errs by up to half a subnormal spacing, 2^-150,
instead (gfx950 kernels keep fp32 subnormals, MFMA included), so the same n + 2 operations add (n + 2) 2^-150 -- below
1e-42 everywhere here and visible only where a sum consists of subnormal terms alone.  Where an operand is itself a
rounded intermediate its own bound is propagated in float64 and ADDED.  No extra factor, no measured slack: a ratio
above 1 is a failure to explain."""
from __future__ import annotations

import numpy as np

U32 = 2.0 ** -24              # fp32 unit roundoff
SUB32 = 2.0 ** -150           # half the spacing of the fp32 subnormals


def sum_bound(n, abs_sum, operand_err=0.0):
    """(n + 2) (u sum |t_i| + 2^-150) (+ the propagated error of rounded operands); n broadcasts against abs_sum"""
    return (np.asarray(n, dtype=np.float64) + 2.0) * (U32 * np.asarray(abs_sum, dtype=np.float64) + SUB32) + operand_err


def element_check(name, got, ref64, bound, report):
    """Every element on its own: |got - ref64| <= bound (an element with bound 0 must be exact; NaN / inf never pass).
    Keeps the worst err / bound in report[name]; returns the failure lines (empty list: every element passes)."""
    got = np.asarray(got, dtype=np.float64)
    ref64 = np.asarray(ref64, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref64.shape)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - ref64)
        ratio = np.where(err == 0, 0.0, err / bound)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    worst = float(ratio.max(initial=0.0))
    report[name] = max(report.get(name, 0.0), worst)
    bad = ~(err <= bound)
    if not bad.any():
        return []
    flat = np.flatnonzero(bad)
    top = flat[np.argsort(-ratio.reshape(-1)[flat])][:4]
    where = ", ".join(f"{tuple(int(x) for x in np.unravel_index(i, ref64.shape))}: got {got.reshape(-1)[i]!r} ref "
                      f"{ref64.reshape(-1)[i]!r} err/bound {ratio.reshape(-1)[i]:.3g}" for i in top)
    return [f"{name}: {int(bad.sum())} of {bad.size} elements over the bound; worst: {where}"]


def fmt_report(report):
    return " ".join(f"{k}={v:.3f}" for k, v in report.items())


# ---- window pairs and the float64 scatter reference -------------------------------------------------------------------
def window_pairs(offsets, items, users, ends, end_delta, L, pad_key):
    """(keys, vals, lens) as gbwd_pairs_kernel writes them: state-major, L slots per state, the window's items first,
    pad_key behind them; vals = the state; window = items[o + end - len, o + end), end = ends + end_delta,
    len = min(end, L)."""
    offsets, items = np.asarray(offsets, dtype=np.int64), np.asarray(items, dtype=np.int64)
    users = np.asarray(users, dtype=np.int64)
    end = np.asarray(ends, dtype=np.int64) + int(end_delta)
    assert np.all(end >= 0) and np.all(end <= offsets[users + 1] - offsets[users]), "window outside the user's row"
    lens = np.minimum(end, L)
    j = np.arange(L)[None, :]
    idx = (offsets[users] + end - lens)[:, None] + j
    valid = j < lens[:, None]
    keys = np.where(valid, items[np.where(valid, idx, 0)], pad_key)
    vals = np.broadcast_to(np.arange(len(users))[:, None], keys.shape)
    return keys.reshape(-1), vals.reshape(-1).copy(), lens


def segsum_reference(keys, terms64, n_rows):
    """(sum, sum of absolute values, number of terms) per key < n_rows, in float64"""
    keys = np.asarray(keys, dtype=np.int64)
    live = keys < n_rows
    ref = np.zeros((n_rows,) + terms64.shape[1:])
    ab = np.zeros_like(ref)
    np.add.at(ref, keys[live], terms64[live])
    np.add.at(ab, keys[live], np.abs(terms64[live]))
    return ref, ab, np.bincount(keys[live], minlength=n_rows)


def gather_bwd_reference(dh0, offsets, items, users, ends, end_delta, L, n_items):
    """g_E_in[item] = sum over the windows that hold it of dh0[state] / len_state, float64, with the element bound: the
    row's n terms carry one rounding each (the division).  Returns (ref [n_items, d], bound, cnt [n_items])."""
    keys, vals, lens = window_pairs(offsets, items, users, ends, end_delta, L, n_items)
    terms = np.asarray(dh0, dtype=np.float32).astype(np.float64)[vals] / np.maximum(lens, 1)[vals][:, None]
    ref, ab, cnt = segsum_reference(keys, terms, n_items)
    return ref, sum_bound(cnt[:, None], ab), cnt


def onehot_reference(coef, act, hb, n_items):
    """g_E_out[a] = sum_{b: act[b] = a} coef[b] hb[b] and g_b_out[a] = sum coef[b] in float64 with their element bounds
    (n = the action's count; a term = one product, the bias terms carry no rounding).  Returns (refE, boundE, refb,
    boundb, cnt)."""
    coef = np.asarray(coef, dtype=np.float32).astype(np.float64)
    hb = np.asarray(hb, dtype=np.float32).astype(np.float64)
    act = np.asarray(act, dtype=np.int64)
    refE, abE, cnt = segsum_reference(act, coef[:, None] * hb, n_items)
    refb, abb, _ = segsum_reference(act, coef[:, None], n_items)
    return refE, sum_bound(cnt[:, None], abE), refb[:, 0], sum_bound(cnt, abb[:, 0]), cnt


# ---- the one-hot case: the catalogue / batch pair of test_gpu_lean_update.py; the seed is chosen for its hot actions ------
OH_U, OH_N, OH_B, OH_L, OH_SEED = 2000, 40, 256, 10, 22


def onehot_case_log():
    """(offsets, items, rewards): helpers.small_log(U=2000, N=40, seed=3, mean_len=14, max_len=45)"""
    from oracle import cql_oracle as O
    u, i, t, r = O.synth_log(OH_U, OH_N, seed=3, mean_len=14, max_len=45)
    return O.build_csr(u, i, t, r, OH_U)


def onehot_case_actions():
    """the actions the sampler draws at step 0 (sample_positions is the sampler's oracle, bit-exact by test_gpu_kernels)"""
    from oracle import cql_oracle as O
    off, items, _ = onehot_case_log()
    return items[O.sample_positions(OH_SEED, 0, 0, OH_B, int(off[-1]))]


def onehot_case_is_hot(act):
    """at least three actions repeat 9 times or more (their runs cross the 8-pair chunks), one more than 64 times, and
    some action is never sampled"""
    cnt = np.bincount(np.asarray(act, dtype=np.int64), minlength=OH_N)
    return bool((cnt >= 9).sum() >= 3 and cnt.max() > 64 and (cnt == 0).any())


# ---- crafted key layouts (L = 1, one state per user, one item per user: the sorted keys are the per-item counts) -------
# Run lengths in item-id order.  Last pair of a run at 64q - 1 (63, 127, 191, 319, 575, 639, 1599, 2239, 2302), at 64q
# (128, 384, 576, 2304) and at 64q + 1 (577); runs of exactly one ([0, 64), [64, 128)), two ([192, 320)) and ten
# ([1600, 2240)) whole chunks; a 640-run that starts mid-chunk (902); a run of two on the last pair of chunk 35 and the
# first of chunk 36 (2303, 2304).  2310 pairs = 36 chunks of 64 and 6 pairs.
RUN_COUNTS = (64, 64, 1, 63, 128, 65, 191, 1, 1, 62, 259, 3, 640, 5, 53, 640, 63, 2, 5)
HOT_RUNS = (12, 15)          # positions in RUN_COUNTS of the 640-runs: mid-chunk start; ten whole chunks
PAIR_RUN = 17                # position of the run of two that crosses a chunk edge


def crafted_layout(name, seed=0):
    """dict(items [n_states] the one item of state i's user, ends [n_states] 1 or 0 (empty state), n_items, run_ids: the
    item id of every RUN_COUNTS run (None for the layouts that have none)).  Every third item id gets no pair.
        runs      the 2310 pairs above                       37 chunks: 3 idle waves in the last block
        pad_mid   + 140 empty states: padding starts at 2310, mid-chunk; chunks 37 and 38 all padding
                                                             39 chunks: 1 idle wave
        pad_edge  the last 6 pairs' states emptied + 90 empty states: padding starts at 2304 = 36 x 64
                                                             38 chunks: 2 idle waves
        all_empty 300 states, every one empty
        one_item  n_items = 1: one run over 663 pairs, 37 empty states
        pow2      n_items = 64 (pad key 64 = 2^6: one more key bit than the items), 500 states, 40 empty
        pow2m1    n_items = 63 (pad key 63: every key bit set)"""
    rng = np.random.default_rng(seed)
    run_ids = None
    if name in ("runs", "pad_mid", "pad_edge"):
        run_ids = np.array([i + i // 2 for i in range(len(RUN_COUNTS))], dtype=np.int64)   # 0 1 3 4 6 7 ...: gaps
        items = np.repeat(run_ids, RUN_COUNTS)
        ends = np.ones(items.size, dtype=np.int32)
        n_items = int(run_ids[-1]) + 3
        if name == "pad_edge":
            ends[-6:] = 0
        extra = {"runs": 0, "pad_mid": 140, "pad_edge": 90}[name]
        items = np.concatenate([items, rng.integers(0, n_items, extra)])
        ends = np.concatenate([ends, np.zeros(extra, np.int32)])
    elif name == "all_empty":
        n_items, items, ends = 50, rng.integers(0, 50, 300), np.zeros(300, np.int32)
    elif name == "one_item":
        n_items, items = 1, np.zeros(700, dtype=np.int64)
        ends = np.ones(700, np.int32)
        ends[rng.choice(700, 37, replace=False)] = 0
    elif name in ("pow2", "pow2m1"):
        n_items = 64 if name == "pow2" else 63
        items = rng.integers(0, n_items, 500)
        items[:3] = (n_items - 1, 0, n_items - 1)
        ends = np.ones(500, np.int32)
        ends[rng.choice(np.arange(3, 500), 40, replace=False)] = 0
    else:
        raise ValueError(name)
    perm = rng.permutation(items.size)                     # the sort has work to do; stable: state order inside a run
    return dict(items=items[perm].astype(np.int32), ends=ends[perm], n_items=n_items, run_ids=run_ids)


CRAFTED = ("runs", "pad_mid", "pad_edge", "all_empty", "one_item", "pow2", "pow2m1")


def layout_log(lay):
    """(offsets, items, users, ends, L) of a crafted layout: user i = state i, one interaction each"""
    n = lay["items"].size
    return np.arange(n + 1, dtype=np.int64), lay["items"], np.arange(n, dtype=np.int32), lay["ends"], 1


WINDOW_CASES = {"L70": (70, 0), "L50d1": (50, 1)}      # a window longer than a wave; next-state windows (end_delta = 1)


def window_case(L, end_delta, seed=3):
    """(offsets, items, users, ends, n_items) of a random Zipf log over 23 items: 90 states with windows of up to L items
    (6300 / 4500 pairs, the hot items' runs span many chunks); ends + end_delta stays inside the user's row, some
    windows are empty (ends + end_delta = 0 needs end_delta = 0), some shorter than L"""
    from oracle import cql_oracle as O
    U, Nn, n = 30, 23, 90
    u, i, t, r = O.synth_log(U, Nn, seed=seed, mean_len=max(9, L), max_len=3 * L + 7)
    off, items, _ = O.build_csr(u, i, t, r, U)
    rng = np.random.default_rng(1)
    users = rng.integers(0, U, n).astype(np.int32)
    cnt = (off[users.astype(np.int64) + 1] - off[users]).astype(np.int64)
    ends = (rng.integers(0, 10**6, n) % (cnt + 1 - end_delta)).astype(np.int32)
    ends[:3] = 0
    return off, items, users, ends, Nn


def sorted_pairs(keys, vals):
    """stable sort by key: what the radix sort leaves"""
    o = np.argsort(keys, kind="stable")
    return keys[o], vals[o]


def segsum_geometry(keys_sorted, pad_key, ch):
    """where the padding starts and how the chunks fall into blocks of 4 waves"""
    n = keys_sorted.size
    live = int(np.searchsorted(keys_sorted, pad_key))
    n_chunks = (n + ch - 1) // ch
    return dict(n_pairs=n, live=live, n_chunks=n_chunks, idle_waves=(-n_chunks) % 4,
                pad_chunks=n_chunks - (live + ch - 1) // ch)


# ---- NumPy port of segsum_pass1_kernel / segsum_pass2_kernel -----------------------------------------------------------
def _sum32(rows, order):
    """fp32 sum of a list of fp32 rows: "kernel" first to last, "reverse" last to first, "pairwise" a balanced tree"""
    if order == "reverse":
        rows = rows[::-1]
    if order == "pairwise":
        rows = list(rows)
        while len(rows) > 1:
            rows = [(rows[i] + rows[i + 1]).astype(np.float32) if i + 1 < len(rows) else rows[i]
                    for i in range(0, len(rows), 2)]
        return rows[0]
    acc = np.zeros_like(rows[0])
    for r in rows:
        acc = (acc + r).astype(np.float32)
    return acc


def segsum_emulate(keys, terms32, n_rows, pad_key, ch, order="kernel", fault=None):
    """The two passes of gbwd.hip in fp32, chunk length `ch`: keys sorted [n] (padding = pad_key at the end), terms32
    [n, d] the fp32 term of every sorted pair.  Pass 1 walks every chunk, sums each piece of a run (`order`) and stores it
    to the run's row, to edge[chunk][0] (the run came in from the left) or to edge[chunk][1] (it leaves to the right and
    started here); pass 2, for the chunk in which a crossing run starts, finds the run's last chunk by binary search and
    sums the pieces (`order`).  Returns dst [n_rows + 1, d] (zero-filled on entry; row n_rows is the pad row).
    fault (for the self-test): ("drop", i) pair i is not added; ("twice", i) pair i is added twice;
    ("edge_to_neighbour", k) the last piece of key k's crossing run goes to the next key's row (the previous key's when
    k is the last one); ("pad_into_last", i) padding pair i is summed into row n_rows - 1."""
    keys = np.asarray(keys, dtype=np.int64)
    terms32 = np.asarray(terms32, dtype=np.float32)
    n, d = terms32.shape
    dst = np.zeros((n_rows + 1, d), dtype=np.float32)
    n_chunks = (n + ch - 1) // ch
    edge = {}
    kind, arg = fault if fault is not None else (None, None)

    def piece(members):
        rows = []
        for i in members:
            if kind == "drop" and i == arg:
                continue
            rows.append(terms32[i])
            if kind == "twice" and i == arg:
                rows.append(terms32[i])
        return _sum32(rows, order) if rows else np.zeros(d, np.float32)

    def key_at(i):
        return int(keys[i]) if i < n else pad_key

    for c in range(n_chunks):
        c0 = c * ch
        if key_at(c0) == pad_key:
            continue                                            # sorted: the whole chunk is padding
        prev_key = key_at(c0 - 1) if c0 > 0 else pad_key
        next_key = key_at(c0 + ch) if c0 + ch < n else pad_key
        run_key = key_at(c0)
        state = {"open_left": run_key == prev_key}

        def flush(open_right, members, run_key=None, c=c, state=state):
            s = piece(members)
            if state["open_left"]:
                edge[(c, 0)] = s
            elif open_right:
                edge[(c, 1)] = s
            else:
                dst[run_key] = s
        members, ended = [], False
        for j in range(ch):
            kj = key_at(c0 + j)
            if kj != run_key:
                flush(False, members, run_key)
                members, run_key = [], kj
                state["open_left"] = False
                if kj == pad_key:
                    ended = True
                    break
            members.append(c0 + j)
        if not ended:
            flush(run_key == next_key, members, run_key)

    for c in range(n_chunks - 1):
        k = key_at(c * ch + ch - 1)
        if k == pad_key or key_at((c + 1) * ch) != k:
            continue                                            # no run leaves this chunk to the right
        if key_at(c * ch) == k and c > 0 and key_at(c * ch - 1) == k:
            continue                                            # the run only passes through
        lo, hi = (c + 1) * ch, n
        while lo < hi:
            mid = (lo + hi) >> 1
            if keys[mid] == k:
                lo = mid + 1
            else:
                hi = mid
        j_end = (lo - 1) // ch
        pieces = [edge[(c, 1)]] + [edge[(j, 0)] for j in range(c + 1, j_end + 1)]
        if kind == "edge_to_neighbour" and k == arg:
            nb = key_at(lo)
            if nb == pad_key:
                nb = int(keys[np.searchsorted(keys, k) - 1])
            dst[nb] = (dst[nb] + pieces.pop()).astype(np.float32)
        dst[k] = _sum32(pieces, order)
    if kind == "pad_into_last":
        assert keys[arg] == pad_key
        dst[n_rows - 1] = (dst[n_rows - 1] + terms32[arg]).astype(np.float32)
    return dst


# ---- encoder backward ---------------------------------------------------------------------------------------------------
def encoder_bwd_reference(dH, zb, h0b, W1b, W2b):
    """float64 from the bf16 operands, with the element bounds.  dA1 = (dH W2) [z > 0] is a rounded fp32 intermediate of
    the kernel (n = d products): its bound eA is carried, in float64, into what is made of it --
        dh0 = dA1 W1           (n = d)     + eA |W1|
        gW1 = dA1^T h0         (n = rows)  + eA^T |h0|
        gb1 = colsum dA1       (n = rows)  + colsum eA
    gW2 = dH^T z and gb2 = colsum dH (n = rows) have exact operands.  Returns {name: (ref, bound)} and the dead rows."""
    dH = np.asarray(dH, dtype=np.float32).astype(np.float64)
    z, h0 = np.asarray(zb, dtype=np.float64), np.asarray(h0b, dtype=np.float64)
    W1, W2 = np.asarray(W1b, dtype=np.float64), np.asarray(W2b, dtype=np.float64)
    rows, d = dH.shape
    mask = z > 0
    dA1 = (dH @ W2) * mask
    eA = sum_bound(d, np.abs(dH) @ np.abs(W2)) * mask
    aA = np.abs(dA1)              # (the kernel sums its own rounded dA1: at most aA + eA in magnitude)
    out = {
        "dh0": (dA1 @ W1, sum_bound(d, (aA + eA) @ np.abs(W1), eA @ np.abs(W1))),
        "gW1": (dA1.T @ h0, sum_bound(rows, (aA + eA).T @ np.abs(h0), eA.T @ np.abs(h0))),
        "gb1": (dA1.sum(0), sum_bound(rows, (aA + eA).sum(0), eA.sum(0))),
        "gW2": (dH.T @ z, sum_bound(rows, np.abs(dH).T @ np.abs(z))),
        "gb2": (dH.sum(0), sum_bound(rows, np.abs(dH).sum(0))),
    }
    return out, ~mask.any(1)


# ---- TD target and loss -------------------------------------------------------------------------------------------------
def td_reference(q_a, lse, q_targ, rew, done, gamma, alpha, inv_batch):
    """float64 from the fp32 inputs and the fp32 scalars, with the bounds of the kernel's expression
        y = rew + gamma (1 - done) q_targ                      three operations: 3 u (|rew| + |gamma (1-done) q_targ|)
        coef = (q_a - y - alpha) inv_batch                     y's error + three more: e_y |inv| + 3 u (|q_a| + |y| + |alpha|) |inv|
        loss = inv_batch sum_b [0.5 delta^2 + alpha (lse - q_a)]   n = B terms; a term's own roundings (delta from the
               rounded y, the square, two products, two differences) are carried as operand error.
    done is 0 or 1, so 1 - done is exact.  Returns dict of (ref, bound)."""
    f = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)       # noqa: E731
    q_a, lse, q_targ, rew, done = f(q_a), f(lse), f(q_targ), f(rew), f(done)
    g, a, inv = float(np.float32(gamma)), float(np.float32(alpha)), float(np.float32(inv_batch))
    with np.errstate(over="ignore", invalid="ignore"):
        boot = np.where(done == 1.0, 0.0, g * (1.0 - done) * q_targ)
        y = rew + boot
        ey = 3.0 * (U32 * (np.abs(rew) + np.abs(boot)) + SUB32)
        delta = q_a - y
        coef = (delta - a) * inv
        ecoef = (ey + 3.0 * U32 * (np.abs(q_a) + np.abs(y) + abs(a))) * abs(inv) + 3.0 * SUB32
        term = 0.5 * delta * delta + a * (lse - q_a)
        # delta carries ey and one rounding of its own; (0.5 delta) delta rounds once; lse - q_a and its product with alpha
        # round once each; so does the sum of the two parts
        ed = ey + U32 * np.abs(delta)
        eterm = np.abs(delta) * ed + 0.5 * ed * ed + U32 * 0.5 * delta * delta + \
            2.0 * U32 * abs(a) * (np.abs(lse) + np.abs(q_a)) + U32 * np.abs(term) + 6.0 * SUB32
        B = q_a.size
        loss = term.sum() * inv
        eloss = (sum_bound(B, np.abs(term).sum(), eterm.sum()) + U32 * abs(term.sum())) * abs(inv)
    return {"y": (y, ey), "coef": (coef, ecoef), "loss": (loss, eloss)}
