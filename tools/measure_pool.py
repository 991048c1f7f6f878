"""The training pool (tafl_pool_ingest / tafl_pool_sample): what an ingest costs and how fast minibatches are drawn.

65 536 Copenhagen lanes x 8 examples, K = 64, 11x11.  The examples are recorded by tafl_selfplay_record from the start position (S = 64,
cap 512) and then finalized against ANOTHER batch of the same size in which every game has been played to its end with random moves, so
that every example counts as finished: the results are meaningless, the bytes an ingest moves are those of a full examples object.
  * tafl_pool_ingest into a pool of 65 536 x 8 rows: HIP events on the context's stream around each call (the three kernels and the
    24-byte read-back), one warm-up, `--launches` timed calls, min..max, and the bytes read from the examples plus the bytes written to
    the pool against the achievable HBM bandwidth (6.3 TB/s, the rate DESIGN.md section 12 uses);
  * tafl_pool_sample with device pointers and symmetries at 4 096 and 65 536 rows, against tafl_examples_gather with device pointers at
    the same row count, random indices and mixed symmetries, in the same process (that kernel is the one of section 12, untouched).

    python tools/measure_pool.py [--games 65536] [--moves 8] [--launches 10] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from alphazeroforhnefatafl_amd import abi  # noqa: E402
from alphazeroforhnefatafl_amd._lib import check, lib  # noqa: E402
from alphazeroforhnefatafl_amd.abi import TaflPoolIngestResult  # noqa: E402
from alphazeroforhnefatafl_amd.engine import BatchedGameLogic  # noqa: E402

HBM_ACHIEVABLE = 6.3e12


def timed(stream, launches, torch, call):
    """µs of `launches` calls after one warm-up, HIP events on the context's stream around each."""
    us = []
    for k in range(launches + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        if k:
            us.append(1e3 * e0.elapsed_time(e1))
    return us


def rate(us, nbytes):
    return {"us": [min(us), max(us)], "bytes": int(nbytes), "gb_per_s": [nbytes / max(us) / 1e3, nbytes / min(us) / 1e3],
            "fraction_of_hbm": [nbytes / (max(us) * 1e-6) / HBM_ACHIEVABLE, nbytes / (min(us) * 1e-6) / HBM_ACHIEVABLE]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--moves", type=int, default=8)
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--cap", type=int, default=512)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    G, moves, K = a.games, a.moves, 64
    lg = BatchedGameLogic(abi.rules.COPENHAGEN, 11, 128)
    n, A = lg.side_len, lg.action_size
    BW = (n * n + 3) // 4
    stream = torch.cuda.ExternalStream(lib().tafl_ctx_stream(lg._h))
    b = lg.new_batch(G, abi.boards.COPENHAGEN)
    ex = lg.new_examples(G, moves, K)
    b.selfplay_record(ex, moves, a.sims, 1.0, 2, a.cap, sample_seed=11, temp_moves=moves, want_plays=False)
    done = lg.new_batch(G, abi.boards.COPENHAGEN)
    done.random_advance(5, (C.c_uint32 * G)(*[100000] * G), 0)               # every game played to its end
    ex.finalize(done)
    b.close(); done.close()
    E = G * moves
    nc_sum = 0
    for e0 in range(0, E, 1 << 16):
        nc_sum += int(ex.read(np.arange(e0, min(E, e0 + (1 << 16)), dtype=np.uint32))[0].sum())
    res = {"games": G, "moves": moves, "max_children": K, "examples": int(ex.counts()[1]), "policy_entries": nc_sum}

    pool = lg.new_pool(E, K)
    out = TaflPoolIngestResult()
    us = timed(stream, a.launches, torch, lambda: check(lib().tafl_pool_ingest(pool._h, ex._h, C.byref(out))))
    T = int(out.taken)
    RW = 4 * ((BW + 5 + K + 3) // 4)
    # read: len, and per entry info and final twice (count and copy pass); per taken example the board words, N, move_no, z and its policy words
    read = 4 * G + 2 * 5 * E + T * (4 * BW + 12) + 4 * nc_sum
    res["ingest"] = dict(rate(us, read + T * 4 * RW), taken=T, skipped_open=int(out.skipped_open), skipped_overflow=int(out.skipped_overflow),
                         bytes_read=int(read), bytes_written=int(T * 4 * RW), row_bytes=4 * RW, pool_device_bytes=int(pool.stats().device_bytes))
    if T == 0:
        raise SystemExit("no example was taken: " + json.dumps(res))

    res["rows"] = []
    rng = np.random.default_rng(1)
    for rows in (4096, 65536):
        boards = torch.empty((rows, n, n), dtype=torch.uint8, device="cuda:0")
        sides = torch.empty(rows, dtype=torch.uint8, device="cuda:0")
        pi = torch.empty((rows, A), dtype=torch.float32, device="cuda:0")
        z = torch.empty(rows, dtype=torch.float32, device="cuda:0")
        fin = torch.empty(rows, dtype=torch.uint8, device="cuda:0")
        slot = torch.empty(rows, dtype=torch.int32, device="cuda:0")
        sym = torch.empty(rows, dtype=torch.uint8, device="cuda:0")
        idx = torch.from_numpy((rng.integers(0, moves, rows) * G + rng.integers(0, G, rows)).astype(np.int32)).cuda()
        mixed = torch.from_numpy(rng.integers(0, 8, rows).astype(np.uint8)).cuda()
        torch.cuda.synchronize()
        vp = C.c_void_p
        step = [0]

        def sample():
            step[0] += 1
            check(lib().tafl_pool_sample(pool._h, 7, step[0], 0, rows, abi.POOL_SAMPLE_SYM, vp(boards.data_ptr()), vp(sides.data_ptr()), vp(pi.data_ptr()),
                                         vp(z.data_ptr()), vp(slot.data_ptr()), vp(sym.data_ptr()), 1))

        def gather():
            check(lib().tafl_examples_gather(ex._h, vp(idx.data_ptr()), vp(mixed.data_ptr()), rows, vp(boards.data_ptr()), vp(sides.data_ptr()),
                                             vp(pi.data_ptr()), vp(z.data_ptr()), vp(fin.data_ptr()), 1))

        res["rows"].append({"rows": rows, "pool_sample": rate(timed(stream, a.launches, torch, sample), rows * (4 * A + n * n + 10)),
                            "examples_gather": rate(timed(stream, a.launches, torch, gather), rows * (4 * A + n * n + 6))})
    for k, v in res.items():
        print(k, json.dumps(v))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
