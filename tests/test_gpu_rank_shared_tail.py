"""cqlrec_split_rank (shuffle = 0) and cqlrec_prepare_rank (key2 = NULL) rank the rows of a user by (key descending, input
row descending) and are documented to agree.  Both end in the one rank tail of csrc/segment_common.hip (user pass, segment
bounds with the gap fill, rank, count): their outputs are byte-equal to each other and equal to the numpy yardstick
split_reference.rank_in_user.  Shapes sit around the 256-thread block (255, 256, 257), span several blocks (1025) and
include the single row; n_users = 300 with few rows leaves long gaps of empty users for one thread to fill."""
import numpy as np
import pytest
import torch

import split_reference as R
from replay_cql_amd import _native as N

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


def _device_ranks(user, key, n_users):
    lib = N.load()
    n = len(user)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    u = torch.as_tensor(user.astype(np.int32)).to(DEV)
    k = torch.as_tensor(key).to(DEV)
    out = {}
    for which in ("split", "prepare"):
        rank = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        count = torch.full((n_users,), -7, dtype=torch.int32, device=DEV)
        if which == "split":
            nb = int(lib.cqlrec_split_rank_ws_bytes(n, n_users))
            ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
            present = torch.full((1,), -7, dtype=torch.int64, device=DEV)
            N.check(lib.cqlrec_split_rank(u.data_ptr(), k.data_ptr(), n, n_users, 0, 0, ws.data_ptr(), nb, rank.data_ptr(),
                                          count.data_ptr(), present.data_ptr(), stream), "split_rank")
            out["present"] = int(present.cpu()[0])
        else:
            nb = int(lib.cqlrec_prepare_rank_ws_bytes(n, n_users))
            ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
            N.check(lib.cqlrec_prepare_rank(u.data_ptr(), k.data_ptr(), None, n, n_users, 0, ws.data_ptr(), nb, rank.data_ptr(),
                                            count.data_ptr(), stream), "prepare_rank")
        out[which] = (rank.cpu().numpy(), count.cpu().numpy())
    return out


def _cases(n_rows, n_users):
    rng = np.random.default_rng(1000 * n_rows + n_users)
    spread = rng.integers(0, n_users, n_rows)
    tied = np.full(n_rows, 42, dtype=np.int64)
    # few distinct values, so ties everywhere, and both ends of int64 (the key is complemented for the descending sort)
    wide = rng.choice(np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX], dtype=np.int64), n_rows)
    wide[0] = I64_MIN
    wide[-1] = I64_MAX if n_rows > 1 else I64_MIN
    return {
        "keys_tied": (spread, tied),
        "keys_int64_ends": (spread, wide),
        "all_rows_on_last_user": (np.full(n_rows, n_users - 1), wide),     # one thread writes n_users offsets
        "all_rows_on_user_0": (np.zeros(n_rows, dtype=np.int64), wide),
    }


@pytest.mark.parametrize("n_users", [1, 2, 300])
@pytest.mark.parametrize("n_rows", [1, 255, 256, 257, 1025])
def test_split_rank_and_prepare_rank_agree_with_each_other_and_numpy(n_rows, n_users):
    for name, (user, key) in _cases(n_rows, n_users).items():
        want_rank, counts = R.rank_in_user(user, key)
        want_count = np.zeros(n_users, dtype=np.int64)
        want_count[:len(counts)] = counts
        got = _device_ranks(user, key, n_users)
        (s_rank, s_count), (p_rank, p_count) = got["split"], got["prepare"]
        assert s_rank.tobytes() == p_rank.tobytes() and s_count.tobytes() == p_count.tobytes(), name
        assert np.array_equal(s_rank, want_rank), name
        assert np.array_equal(s_count, want_count), name
        assert got["present"] == int((want_count > 0).sum()), name
