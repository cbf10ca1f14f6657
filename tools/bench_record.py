"""What the bench tools of the device-fitted models share: the cfg3 log, the timed call, the warm-up plus repeats, and
the record that prints one JSON line per row and rewrites `--out` after every row."""
from __future__ import annotations

import json
import statistics
import time
from pathlib import Path

import torch


def make_log(n_users: int, n_items: int, dev):
    """data.synth_log_device's log flattened to LOG_SCHEMA device columns in a fixed random row order; the timestamp is the
    position inside the user plus a per-user start (a hash of the user id, 0..999): unique inside a user"""
    from replay_cql_amd import data as D
    offsets, items, rewards = D.synth_log_device(n_users, n_items, device=dev)
    lens = offsets[1:] - offsets[:-1]
    user = torch.repeat_interleave(torch.arange(n_users, dtype=torch.int32, device=dev), lens)
    pos = torch.arange(items.numel(), dtype=torch.int64, device=dev) - offsets[user.long()]
    start = D._lsr(D._mix64(torch.arange(n_users, dtype=torch.int64, device=dev)), 1) % 1000
    ts = start[user.long()] + pos
    order = torch.randperm(items.numel(), device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    return {"user_idx": user[order].contiguous(), "item_idx": items[order].contiguous(),
            "timestamp": ts[order].contiguous(), "relevance": rewards[order].to(torch.float64).contiguous()}


def spread(xs):
    return max(xs) - min(xs)


def timed(fn):
    """(seconds on the host clock, what fn returned) of a call between two device synchronises"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def repeat(fn, repeats: int):
    """(the times of `repeats` calls after one warm-up, what the last call returned)"""
    timed(fn)
    times, out = [], None
    for _ in range(repeats):
        out = None                                       # a result still held would make the next call allocate elsewhere
        t, out = timed(fn)
        times.append(t)
    return times, out


class Recorder:
    """Rows go to `calls` (a dict inside `result`) and to stdout, led by the fields of `tag`; `result` goes to `out`."""

    def __init__(self, result: dict, out, calls=None):
        self.result, self.out, self.tag = result, out, {}
        self.calls = result.setdefault("calls", {}) if calls is None else calls

    def save(self):
        if self.out:                                     # after every row: a later call running long loses nothing
            path = Path(self.out)
            path.parent.mkdir(parents=True, exist_ok=True)
            path.write_text(json.dumps(self.result, indent=1) + "\n")

    def record(self, name, times, **more):
        """the row {s, median_s, spread_s, **more} of a call; returns its median"""
        row = {"s": times, "median_s": statistics.median(times), "spread_s": spread(times), **more}
        self.calls[name] = row
        print(json.dumps({**self.tag, "call": name, **{k: v for k, v in row.items() if not isinstance(v, list)}}), flush=True)
        self.save()
        return row["median_s"]
