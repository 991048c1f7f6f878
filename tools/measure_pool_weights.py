"""Weighted sampling of the training pool (tafl_pool_set_weights / tafl_pool_sample_weighted): what the rebuild of
the prefix structure, a priority update and a weighted minibatch cost beside the uniform tafl_pool_sample.

The 524 288-row 11x11 pool of tools/measure_pool.py (65 536 Copenhagen lanes x 8 examples, K = 64, every example counted as finished) and
a second pool of 4 Mi rows filled by ingesting the same examples object eight times.  Every slot gets a random weight, every third one 0.
Per pool, µs per call from HIP events on the context's stream, one warm-up, `--launches` timed calls, min..max:
  * the rebuild (tafl_pool_weight_stats after a trim that removes nothing marked the sums dirty): two kernels and a 16-byte read-back;
  * tafl_pool_set_weights of 4 096 entries with device pointers;
  * tafl_pool_sample_weighted at 4 096 and 65 536 rows with the rebuild already done, and tafl_pool_sample at the same counts,
    alternating in the same process;
  * tafl_pool_set_weights of the slots just served followed by tafl_pool_sample_weighted: the step of prioritised replay, which pays a
    rebuild per minibatch.
--uniform-only times tafl_pool_ingest and tafl_pool_sample alone with weighting off and takes --lib, so that this commit and another
build can take turns as separate processes.

    python tools/measure_pool_weights.py [--launches 10] [--json out.json] [--uniform-only] [--lib path/to/libtaflhip.so]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from alphazeroforhnefatafl_amd import _lib, abi  # noqa: E402


def timed(stream, launches, torch, call):
    us = []
    for k in range(launches + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        if k:
            us.append(1e3 * e0.elapsed_time(e1))
    return [min(us), max(us)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--moves", type=int, default=8)
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--cap", type=int, default=512)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--big", type=int, default=8, help="the second pool holds this many ingests")
    ap.add_argument("--json", default=None)
    ap.add_argument("--uniform-only", action="store_true")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    import torch                                                                # (before any load of the library: one HIP runtime per process)
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
        if a.uniform_only:                                                      # an older build: bind what it exports
            probe = C.CDLL(_lib.LIB_PATH)
            _lib.SYMBOLS[:] = [s for s in _lib.SYMBOLS if hasattr(probe, s[0])]
    from alphazeroforhnefatafl_amd._lib import check, lib
    from alphazeroforhnefatafl_amd.abi import TaflPoolIngestResult
    from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
    G, moves, K = a.games, a.moves, 64
    lg = BatchedGameLogic(abi.rules.COPENHAGEN, 11, 128)
    n, A = lg.side_len, lg.action_size
    stream = torch.cuda.ExternalStream(lib().tafl_ctx_stream(lg._h))
    b = lg.new_batch(G, abi.boards.COPENHAGEN)
    ex = lg.new_examples(G, moves, K)
    b.selfplay_record(ex, moves, a.sims, 1.0, 2, a.cap, sample_seed=11, temp_moves=moves, want_plays=False)
    done = lg.new_batch(G, abi.boards.COPENHAGEN)
    done.random_advance(5, (C.c_uint32 * G)(*[100000] * G), 0)               # every game played to its end
    ex.finalize(done)
    b.close(); done.close()
    E = G * moves
    vp = C.c_void_p
    dev = torch.device("cuda", 0)
    res = {"games": G, "moves": moves, "max_children": K, "lib": _lib.LIB_PATH, "launches": a.launches, "pools": []}

    def outputs(rows):
        return dict(boards=torch.empty((rows, n, n), dtype=torch.uint8, device=dev), sides=torch.empty(rows, dtype=torch.uint8, device=dev),
                    pi=torch.empty((rows, A), dtype=torch.float32, device=dev), z=torch.empty(rows, dtype=torch.float32, device=dev),
                    slot=torch.empty(rows, dtype=torch.int32, device=dev), sym=torch.empty(rows, dtype=torch.uint8, device=dev),
                    weight=torch.empty(rows, dtype=torch.int32, device=dev), total=torch.zeros(1, dtype=torch.int64, device=dev))

    for ingests in (1,) if a.uniform_only else (1, a.big):
        Cp = E * ingests
        pool = lg.new_pool(Cp, K)
        out = TaflPoolIngestResult()
        for _ in range(ingests - 1):
            check(lib().tafl_pool_ingest(pool._h, ex._h, C.byref(out)))
        r = {"capacity": Cp, "ingest_us": timed(stream, a.launches, torch, lambda: check(lib().tafl_pool_ingest(pool._h, ex._h, C.byref(out)))),
             "taken_per_ingest": int(out.taken), "live": int(pool.stats().live), "rows": []}
        step = [0]

        def uniform(o, rows):
            step[0] += 1
            check(lib().tafl_pool_sample(pool._h, 7, step[0], 0, rows, abi.POOL_SAMPLE_SYM, vp(o["boards"].data_ptr()), vp(o["sides"].data_ptr()), vp(o["pi"].data_ptr()),
                                         vp(o["z"].data_ptr()), vp(o["slot"].data_ptr()), vp(o["sym"].data_ptr()), 1))

        if a.uniform_only:
            for rows in (4096, 65536):
                o = outputs(rows)
                torch.cuda.synchronize()
                r["rows"].append({"rows": rows, "pool_sample_us": timed(stream, a.launches, torch, lambda: uniform(o, rows))})
            res["pools"].append(r)
            pool.close()
            continue

        pool.set_weighting(1)
        rng = np.random.default_rng(1)
        for s0 in range(0, Cp, 1 << 20):                                        # a random weight per slot, every third one 0
            k = min(1 << 20, Cp - s0)
            w = rng.integers(1, 2 ** 32 - 1, k, dtype=np.uint64, endpoint=True).astype(np.uint32)
            w[(np.arange(s0, s0 + k) % 3) == 0] = 0
            pool.set_weights(torch.arange(s0, s0 + k, dtype=torch.int32, device=dev), torch.from_numpy(w.view(np.int32)).to(dev), device=True)
        st = pool.weight_stats()
        r.update(total_weight=int(st.total_weight), positive=int(st.positive), weight_device_bytes=int(st.device_bytes), pool_device_bytes=int(pool.stats().device_bytes))

        def rebuild():
            pool.trim(0xFFFFFFFF)                                               # removes nothing, marks the sums dirty
            pool.weight_stats()

        r["rebuild_us"] = timed(stream, a.launches, torch, rebuild)
        sl = torch.from_numpy(rng.integers(0, Cp, 4096).astype(np.int32)).to(dev)
        wt = torch.from_numpy(rng.integers(0, 2 ** 31, 4096).astype(np.int32)).to(dev)
        torch.cuda.synchronize()
        r["set_weights_4096_us"] = timed(stream, a.launches, torch, lambda: check(lib().tafl_pool_set_weights(pool._h, vp(sl.data_ptr()), vp(wt.data_ptr()), 4096, 1)))
        for rows in (4096, 65536):
            o = outputs(rows)
            torch.cuda.synchronize()

            def weighted():
                step[0] += 1
                check(lib().tafl_pool_sample_weighted(pool._h, 7, step[0], 0, rows, abi.POOL_SAMPLE_SYM, vp(o["boards"].data_ptr()), vp(o["sides"].data_ptr()),
                                                      vp(o["pi"].data_ptr()), vp(o["z"].data_ptr()), vp(o["slot"].data_ptr()), vp(o["sym"].data_ptr()),
                                                      vp(o["weight"].data_ptr()), vp(o["total"].data_ptr()), 1))

            def replay_step():                                                  # new priorities for the rows just served, then the next minibatch
                check(lib().tafl_pool_set_weights(pool._h, vp(o["slot"].data_ptr()), vp(o["weight"].data_ptr()), rows, 1))
                weighted()

            pool.weight_stats()                                                 # the rebuild is done
            w_us, u_us = [], []
            for _ in range(a.launches + 1):                                     # alternating; the first pair is the warm-up
                w_us.append(timed(stream, 1, torch, weighted)[0])
                u_us.append(timed(stream, 1, torch, lambda: uniform(o, rows))[0])
            r["rows"].append({"rows": rows, "sample_weighted_us": [min(w_us[1:]), max(w_us[1:])], "pool_sample_us": [min(u_us[1:]), max(u_us[1:])],
                              "set_weights_then_sample_weighted_us": timed(stream, a.launches, torch, replay_step)})
        r["rebuilds"] = int(pool.weight_stats().rebuilds)
        res["pools"].append(r)
        pool.close()
    for k, v in res.items():
        print(k, json.dumps(v))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
