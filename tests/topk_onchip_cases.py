"""Case tables and host-side builders of the one-pass d = 128 top-K tests (qtopk2_kernel / qtopk4_kernel): shared by
test_gpu_topk_onchip.py (the kernels) and test_topk_onchip_cases_cpu.py (an exact fp32 top-k standing in for them).  The
tables are explained in the docstring of test_gpu_topk_onchip.py."""
import numpy as np

from helpers import _inputs, _row, build_case, topk_inputs

D = 128
CHAIN = (1, 5, 10, 11, 16)
SHARE_CAP = 0.10
ORACLE_KINDS = ("flat1", "flat3", "dyadic")          # exact in every summation order: bit-identical to O.topk_rows

#           id        users  n_cand  kind        seen   ks
CASES_A = [
    ("p_5003",    300,   5003, "plain",    True,  CHAIN),
    ("n_40k",     257,  40000, "neg",      True,  CHAIN),
    ("s_5003",    300,   5003, "straddle", True,  CHAIN),
    ("w_40k",      64,  40000, "wide",     True,  CHAIN),
    ("r_5003",    300,   5003, "ramp",     True,  CHAIN),
    ("d_5003",    300,   5003, "down",     True,  CHAIN),
    ("p_100",     255,    100, "plain",    True,  CHAIN),
    ("p_64",       33,     64, "plain",    False, CHAIN),
    ("p_65",       33,     65, "plain",    False, CHAIN),
    ("p_5",        33,      5, "plain",    True,  CHAIN),
    ("p_1",         1,      1, "plain",    False, CHAIN),
    ("f1",         70,   5003, "flat1",    True,  CHAIN),
    ("f3",         70,   5003, "flat3",    True,  CHAIN),
    ("y_5003",    300,   5003, "dyadic",   True,  (10, 16)),
]

Q4_USERS = 512 * 160 + 300       # the smallest launch the default dispatch gives qtopk4_kernel, plus a partial block
# where the crafted seen rows sit (users base .. base + 10): wave 0 of block 0 (also inside the 700 users of the
# cross-kernel run), wave 2 of block 77, the partly filled third wave of the partial last block
Q4_BASES = (0, 512 * 77 + 256, 512 * 160 + 256)
Q4_CROSS = 700                   # users of the second, qtopk2_kernel, call
LISTS, BITMAP, NO_SEEN = 0, 1, -1

#           id           n_cand  kind        seen load   ks        form
CASES_B = [
    ("q4_light",     5003, "plain",    "light",    (10, 16), LISTS),
    ("q4_ramp",      5003, "ramp",     "light",    (10, 16), LISTS),
    ("q4_neg_1s",     700, "neg",      "light",    (5, 11),  LISTS),
    ("q4_popular",   5003, "straddle", "popular",  (10, 16), LISTS),
    ("q4_heavy",      700, "wide",     "heavy",    (10, 16), BITMAP),
    ("q4_noseen",    5003, "plain",    "none",     (1, 16),  NO_SEEN),
    ("q4_flat3",      700, "flat3",    "light",    (10, 16), LISTS),
]
Q4_PHASE_CASES = ("q4_light", "q4_heavy")


def build_a_case(case):
    cid, n_users, n_cand, kind, with_seen, _ = case
    return build_case(cid, D, n_cand, "identity", kind, n_users, with_seen)


def _q4_checked_users(rng, n):
    crafted = np.concatenate([np.arange(b, b + 11) for b in Q4_BASES])
    us = np.unique(np.concatenate([np.arange(0, 4), [127, 128, 511, 512, 65535, 65536], np.arange(n - 302, n),
                                   rng.integers(0, n, 400), crafted]))
    return us.astype(np.int64), crafted.astype(np.int64)


def build_q4_case(cid, n_cand, kind, load):
    """Host side of a row of table B: Q4_USERS independent users, the whole catalogue (candidate row = id), a seen CSR with
    more rows than users reached through a non-monotone seen_rows map with shared rows.  Returns the operands of the
    launch and, for the checked users `us` only, the fp32 scores S and the admissibility mask (as build_case gives them
    for every user).

    seen loads (rows of users that own their row; a user that shares a row sees what its owner has seen):
      light    0..7 random ids (some past the catalogue) per user; the checked users also 3..7 of their best items
      popular  light + items 3, 40 (one stage) and n_cand - 300 seen by 97 % of the users; every id of CSR rows < 300 twice
      heavy    light + a random half of the catalogue per user (ids past the catalogue are dropped)
      none     no seen CSR at all
    and in every load the crafted rows of _seen_rows at users base + 0, 3..10 of each base in Q4_BASES: lengths 0, 1, 511,
    512, 513, 3 000 (half of each the user's best items), the best n_cand - 40 items, all but 5, all; users base + 1 and
    base + 2 share a row."""
    seed = sum(map(ord, cid)) * 7 + D
    rng = np.random.default_rng(seed)
    n = Q4_USERS
    us, crafted = _q4_checked_users(rng, n)
    if kind == "straddle":         # topk_inputs' shift, taken over the checked users (the dense score matrix of all is 1.6 GB)
        Hb, Eb, b = topk_inputs("plain", n, n_cand, D, seed)
        S = Hb[us] @ Eb.T + b
        kth = -np.partition(-S, 15, axis=1)[:, 15]
        b = (b - np.float32(np.median(kth))).astype(np.float32)
    else:
        Hb, Eb, b = _inputs(kind, n, n_cand, D, seed)
    S = (Hb[us] @ Eb.T + b).astype(np.float32)
    c = dict(Hb=Hb, E_c=Eb, b_c=b, ids=np.arange(n_cand, dtype=np.int64), us=us, S=S, kind=kind, seen=None, rows=None,
             mask=None, crafted=crafted)
    if load == "none":
        return c

    n_rows = n + 7
    rows_of = rng.permutation(n_rows)[:n].astype(np.int32)
    owner = np.ones(n, bool)
    for base in Q4_BASES:
        rows_of[base + 2] = rows_of[base + 1]
        owner[base + 2] = False
    rows_of[20000:20100] = rows_of[300:400][::-1]           # more shared rows, among them users of the cross-kernel run
    owner[20000:20100] = False
    plain = owner.copy()                                    # owners whose row is not a crafted one
    plain[crafted] = False
    wide = n_cand + 8                                       # key = CSR row * wide + id; ids up to n_cand + 7

    cnt = np.where(plain, rng.integers(0, 8, n), 0)
    keys = [np.repeat(rows_of.astype(np.int64), cnt) * wide + rng.integers(0, wide, int(cnt.sum()))]
    pos_in_us = {int(u): j for j, u in enumerate(us)}
    for j, u in enumerate(us):                              # the checked users have seen some of their best items
        if plain[u]:
            top = np.argsort(-S[j], kind="stable")[: 3 + (u % 5)]
            keys.append(int(rows_of[u]) * wide + top.astype(np.int64))
    if load == "popular":
        for item in (3, 40, n_cand - 300):
            who = np.nonzero(plain & (rng.random(n) < 0.97))[0]
            keys.append(rows_of[who].astype(np.int64) * wide + item)
    lens = {0: 0, 3: 1, 4: 511, 5: 512, 6: 513, 7: 3000}
    for base in Q4_BASES:
        for o in (0, 1, 3, 4, 5, 6, 7, 8, 9, 10):
            u = base + o
            best = np.argsort(-S[pos_in_us[u]], kind="stable")
            if o >= 8:
                row = _row(rng, best, n_cand, n_cand - {8: 40, 9: 5, 10: 0}[o], 10)
            else:
                ln = min(lens.get(o, 20), n_cand)
                row = _row(rng, best, n_cand, ln // 2, ln - ln // 2)
            keys.append(int(rows_of[u]) * wide + row.astype(np.int64))
    key = np.unique(np.concatenate(keys))
    rows, items = key // wide, (key % wide).astype(np.int32)
    if load == "heavy":
        M = rng.integers(0, 2, (n_rows, n_cand), dtype=np.uint8)
        M[rows_of[crafted]] = 0
        inside = items < n_cand
        M[rows[inside], items[inside]] = 1
        rows, items = np.nonzero(M)
        items = items.astype(np.int32)
        del M
    if load == "popular":                                   # ids repeated in a list (still ascending) count once
        rep = np.where(rows < 300, 2, 1)
        rows, items = np.repeat(rows, rep), np.repeat(items, rep)
    off = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=off[1:])
    mask = np.zeros(S.shape, bool)
    for j, u in enumerate(us):
        r = items[off[rows_of[u]]: off[rows_of[u] + 1]]
        mask[j, r[r < n_cand]] = True
    c.update(seen=(off, items), rows=rows_of, mask=mask)
    return c


def q4_subset(c):
    """the case restricted to its checked users, in the form _oracle / the certificate take"""
    us = c["us"]
    return dict(Hb=c["Hb"][us], E_c=c["E_c"], b_c=c["b_c"], ids=c["ids"], seen=c["seen"],
                rows=None if c["rows"] is None else c["rows"][us], mask=c["mask"], S=c["S"], kind=c["kind"])


def q4_crafted_admissible(c):
    """admissible items of users base + 8, 9, 10 of every base: [len(Q4_BASES), 3]"""
    pos = np.searchsorted(c["us"], np.add.outer(np.asarray(Q4_BASES), np.arange(8, 11)))
    return (~c["mask"]).sum(1)[pos]
