"""Self-play that records training examples on the device (include/taflhip.h tafl_selfplay_record / tafl_examples_*, DESIGN.md section
12) on a real MI355X: the recording kernel against the second route through the library {mcts_run; root_children; Python pick;
encode_boards; tafl_step} for every game and against the oracle loop of tests/examples_util.py for spot ids; the invariances every search
variant here is held to; capacity by bookkeeping; the minibatch gather with device and host pointers.  `pytest -m gpu`."""
import ctypes as C
import random

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflPlay, TaflState
from oracle import oracle as orc
from tests import examples_util as xu
from tests import parity_util as pu

pytestmark = pytest.mark.gpu

_LOGICS = {}


def gpu_logic(rules, n, wb):
    from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
    key = (bytes(rules.to_c()), n, wb)
    if key not in _LOGICS:
        _LOGICS[key] = BatchedGameLogic(rules, n, wb)
    return _LOGICS[key]


def _mk(name):
    rules, fen, wb = pu.CONFIGS[name]
    n = abi.fen_side_len(fen)
    return rules, fen, wb, n, orc.GameLogic(rules, n), gpu_logic(rules, n, wb)


def _start(glg, fen, G, base, mod=30):
    a = glg.new_batch(G, fen)
    plies = (C.c_uint32 * G)(*[(i * 5) % mod for i in range(G)])
    a.random_advance(2, plies, base)
    return a, a.download()


def _batch(glg, states, G, first=0):
    b = glg.new_batch(G)
    b.upload((TaflState * G).from_buffer_copy(bytes(states)[first * C.sizeof(TaflState):(first + G) * C.sizeof(TaflState)]))
    return b


FIELDS = ("nc", "overflow", "played", "move_no", "acts", "vis", "boards", "sides", "z", "fin")


def snapshot(ex, G, rows, n, with_pi=False):
    """Every example of `ex` as arrays [rows, G, ...] (zero where a game has no example j), + lens."""
    lens, total = ex.counts()
    lens = np.frombuffer(lens, np.uint32).copy()
    assert total == int(lens.sum()) and lens.max(initial=0) <= rows
    jj, gg = np.nonzero(np.arange(rows)[:, None] < lens[None, :])
    idx = (jj * G + gg).astype(np.uint32)
    K = ex.max_children
    S = {"lens": lens, "nc": np.zeros((rows, G), np.uint32), "overflow": np.zeros((rows, G), np.uint8), "played": np.zeros((rows, G), np.uint32),
         "move_no": np.zeros((rows, G), np.uint32), "acts": np.zeros((rows, G, K), np.uint32), "vis": np.zeros((rows, G, K), np.uint32),
         "boards": np.zeros((rows, G, n, n), np.uint8), "sides": np.zeros((rows, G), np.uint8), "z": np.zeros((rows, G), np.float32),
         "fin": np.zeros((rows, G), np.uint8)}
    if idx.size:
        nc, ov, pl, mv, acts, vis = ex.read(idx)
        boards, sides, _, z, fin = _gather_no_pi(ex, idx)
        for name, val in zip(FIELDS, (nc, ov, pl, mv, acts, vis, boards, sides, z, fin)):
            S[name][jj, gg] = val
    return S


def _gather_no_pi(ex, idx):
    """Examples.gather without the dense policy rows (host pointers; pi = NULL)."""
    from alphazeroforhnefatafl_amd._lib import check, lib
    n, k, vp = ex.logic.side_len, int(idx.size), C.c_void_p
    boards, sides, z, fin = np.zeros((k, n, n), np.uint8), np.zeros(k, np.uint8), np.zeros(k, np.float32), np.zeros(k, np.uint8)
    check(lib().tafl_examples_gather(ex._h, idx.ctypes.data_as(vp), None, k, boards.ctypes.data_as(vp), sides.ctypes.data_as(vp), None,
                                     z.ctypes.data_as(vp), fin.ctypes.data_as(vp), 0))
    return boards, sides, None, z, fin


def same(A, B, where=""):
    assert np.array_equal(A["lens"], B["lens"]), (where, "lens", int(np.flatnonzero(A["lens"] != B["lens"])[0]))
    for f in FIELDS:
        if not np.array_equal(A[f], B[f]):
            bad = np.argwhere(A[f] != B[f])[0]
            raise AssertionError((where, f, bad.tolist(), A[f][tuple(bad)], B[f][tuple(bad)]))


def library_loop(a, G, n, sims, cap, n_moves, seed, base, sample_seed, temp_moves, move_base=0, K=64):
    """The route tafl_selfplay_record replaces, through the library's synchronous entry points, with the pick rule restated in numpy:
    advances batch `a`; returns (plays [n_moves, G] as uint32 words, snapshot-shaped arrays)."""
    S = {"lens": np.zeros(G, np.uint32), "nc": np.zeros((n_moves, G), np.uint32), "overflow": np.zeros((n_moves, G), np.uint8),
         "played": np.zeros((n_moves, G), np.uint32), "move_no": np.zeros((n_moves, G), np.uint32), "acts": np.zeros((n_moves, G, K), np.uint32),
         "vis": np.zeros((n_moves, G, K), np.uint32), "boards": np.zeros((n_moves, G, n, n), np.uint8), "sides": np.zeros((n_moves, G), np.uint8),
         "z": np.zeros((n_moves, G), np.float32), "fin": np.zeros((n_moves, G), np.uint8)}
    plays_all = np.zeros((n_moves, G), np.uint32)
    ar = np.arange(G)
    for m in range(n_moves):
        a.mcts_run(sims, 1.0, seed, cap, game_id_base=base, sim_offset=m * sims)
        kids, cnt = a.mcts_root_children(K)
        rec, cnt = pu.children_view(kids, cnt, G, K)
        st = a.download()
        status, side = pu.state_field(st, G, "status").copy(), pu.state_field(st, G, "side_to_play").copy()
        boards = np.frombuffer(a.encode_boards(), np.uint8).reshape(G, n, n)
        used = np.arange(K)[None, :] < cnt[:, None]
        vis = np.where(used, rec["visits"], 0).astype(np.int64)
        N = vis.sum(axis=1)
        pick = vis.argmax(axis=1)                                   # first maximum
        M = move_base + m
        if M < temp_moves:
            r = np.array([xu.sample_word(sample_seed, base + g, M) for g in range(G)], np.uint64)
            k = ((r * N.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
            pick = (np.cumsum(vis, axis=1) > k[:, None]).argmax(axis=1)
        act = (N > 0) & (status == abi.ONGOING)
        assert (S["lens"][act] == m).all()                          # a game records from its first move until it is over
        S["lens"][act] += 1
        S["nc"][m, act] = cnt[act]
        S["played"][m, act] = rec["action"][ar, pick][act]
        S["move_no"][m, act] = M
        S["acts"][m, act] = np.where(used, rec["action"], 0)[act]
        S["vis"][m, act] = vis[act]
        S["boards"][m, act] = boards[act]
        S["sides"][m, act] = side[act]
        words = np.where(act, rec["play"][ar, pick], 0).astype(np.uint32)
        plays_all[m] = words
        a.do_play((TaflPlay * G).from_buffer_copy(words.tobytes()), want_effects=False)
    st = a.download()
    status, winner = pu.state_field(st, G, "status"), pu.state_field(st, G, "winner")
    rec_mask = np.arange(n_moves)[:, None] < S["lens"][None, :]
    z = np.where(status[None, :] == 1, np.where(winner[None, :] == S["sides"], 1.0, -1.0), np.where(status[None, :] == 2, 1e-4, 0.0)).astype(np.float32)
    S["z"] = np.where(rec_mask, z, 0).astype(np.float32)
    S["fin"] = np.where(rec_mask & (status[None, :] != abi.ONGOING), 1, 0).astype(np.uint8)
    return plays_all, S


def _plays_words(plays, n_moves, G):
    return np.frombuffer(plays, np.uint32).reshape(n_moves, G)


def _word_tuple(p):
    """A TaflPlay read as a little-endian word -> pu.play_tuple4's (from_row, from_col, axis, disp)."""
    p = int(p)
    d = (p >> 24) & 0xFF
    return (p & 0xFF, (p >> 8) & 0xFF, (p >> 16) & 0xFF, d - 256 if d > 127 else d)


def _check_spots(S, n, ids, want_ex, want_plays, plays, K):
    """Snapshot entries of the games `ids` against the oracle loop's examples (and plays)."""
    for i, g in enumerate(ids):
        assert S["lens"][g] == len(want_ex[i]), (g, S["lens"][g], len(want_ex[i]))
        for j, e in enumerate(want_ex[i]):
            k = len(e.actions)
            got = (S["boards"][j, g].tolist(), int(S["sides"][j, g]), S["acts"][j, g, :k].tolist(), S["vis"][j, g, :k].tolist(), int(S["played"][j, g]), int(S["move_no"][j, g]))
            assert int(S["nc"][j, g]) == k and got == e.fields(), (g, j, got, e.fields())
            assert S["z"][j, g] == e.z and S["fin"][j, g] == e.final, (g, j)
        for m, row in enumerate(want_plays):
            assert _word_tuple(plays[m, g]) == row[i], (g, m)


def _sub_states(states, ids):
    out = (TaflState * len(ids))()
    for i, g in enumerate(ids):
        C.memmove(C.byref(out, i * C.sizeof(TaflState)), C.byref(states[g]), C.sizeof(TaflState))
    return out


SETTINGS = [("copenhagen11", 4096, 32, 5, 160), ("brandubh7", 2048, 40, 12, 64), ("copenhagen13", 512, 16, 3, 96)]
SEED, BASE, SSEED, K = 6, 900, 11, 64


@pytest.mark.parametrize("name,G,sims,n_moves,cap", SETTINGS)
def test_record_equals_the_host_loop(name, G, sims, n_moves, cap):
    """k_mcts_tree_selfplay_rec + k_examples_finalize == the synchronous route through the library for ALL games (plays, final states,
    every example field, len, z) and == the oracle loop for 8 spot ids, with temp_moves = 0, 4 and n_moves; no fault, nothing dropped."""
    rules, fen, wb, n, lg, glg = _mk(name)
    a0, states = _start(glg, fen, G, BASE)
    a0.close()
    ids = sorted({0, 7, 63, 64, G // 2 - 1, G // 2, G - 2, G - 1})
    for temp_moves in (0, 4, n_moves):
        a = _batch(glg, states, G)
        want_plays, want = library_loop(a, G, n, sims, cap, n_moves, SEED, BASE, SSEED, temp_moves, 0, K)
        b = _batch(glg, states, G)
        ex = glg.new_examples(G, n_moves, K)
        plays = _plays_words(b.selfplay_record(ex, n_moves, sims, 1.0, SEED, cap, game_id_base=BASE, sample_seed=SSEED, temp_moves=temp_moves), n_moves, G)
        stats = b.mcts_stats()
        assert stats.faults == 0
        ex.finalize(b)
        where = (name, temp_moves)
        assert np.array_equal(plays, want_plays), (where, np.argwhere(plays != want_plays)[0].tolist())
        fa, fb = a.download(), b.download()
        assert pu.states_equal(fa, fb, G), (where, pu.first_state_diff(fa, fb, G))
        S = snapshot(ex, G, n_moves, n)
        same(S, want, where)
        es = ex.stats()
        assert (es.dropped, es.overflowed, es.bad_index) == (0, 0, 0) and es.device_bytes > 0
        if temp_moves:
            first_max = S["vis"].argmax(axis=2)
            sampled = (S["played"] != np.take_along_axis(S["acts"], first_max[:, :, None], axis=2)[:, :, 0]) & (S["nc"] > 0)
            assert sampled[:min(temp_moves, n_moves)].sum() > G // 4 and not sampled[temp_moves:].any()      # the draw really differs from the argmax
        # the oracle loop on the spot ids
        sub = _sub_states(states, ids)
        o_plays, o_ex, info = xu.oracle_record(orc, lg, sub, len(ids), wb, sims, cap, 1.0, SEED, BASE, n_moves, SSEED, temp_moves, 0,
                                               ids=[BASE + g for g in ids])
        assert info["widest"] < min(sims, K)
        _check_spots(S, n, ids, o_ex, o_plays, plays, K)
        for i, g in enumerate(ids):
            assert bytes(sub[i]) == bytes(fb[g]), (where, g)
        for h in (a, b, ex):
            h.close()


def test_temp_moves_zero_equals_selfplay_run():
    """temp_moves == 0 (with and without an examples object) == tafl_selfplay_run on the same batch: plays, states, simulations."""
    rules, fen, wb, n, lg, glg = _mk("brandubh7")
    G, sims, n_moves, cap = 2048, 40, 12, 64
    a, states = _start(glg, fen, G, BASE)
    want = _plays_words(a.selfplay_run(n_moves, sims, 1.0, SEED, cap, game_id_base=BASE), n_moves, G)
    fa, sa = a.download(), a.mcts_stats()
    for with_ex in (True, False):
        b = _batch(glg, states, G)
        ex = glg.new_examples(G, n_moves, K) if with_ex else None
        got = _plays_words(b.selfplay_record(ex, n_moves, sims, 1.0, SEED, cap, game_id_base=BASE, sample_seed=77, temp_moves=0), n_moves, G)
        assert np.array_equal(got, want)
        assert pu.states_equal(fa, b.download(), G)
        sb = b.mcts_stats()
        assert (sb.sims, sb.rollouts, sb.rollout_plies, sb.terminal_hits, sb.faults) == (sa.sims, sa.rollouts, sa.rollout_plies, sa.terminal_hits, 0)
        if ex is not None:
            lens, total = ex.counts()
            assert total == int((want != 0).sum())               # one example per play made
            ex.close()
        b.close()


def test_invariance_slots_partitions_shards():
    """Identical examples, plays and states for 1 / 4 / 8 playout slots, 1 / 2 partitions, and two half batches with game_id_base 0 and
    G / 2 against the whole."""
    rules, fen, wb, n, lg, glg = _mk("copenhagen11")
    G, sims, n_moves, cap, base = 2048, 24, 4, 128, 0
    a0, states = _start(glg, fen, G, base)
    a0.close()

    def run(first, cnt, flags):
        b = _batch(glg, states, cnt, first)
        ex = glg.new_examples(cnt, n_moves, K)
        plays = _plays_words(b.selfplay_record(ex, n_moves, sims, 1.0, SEED, cap, game_id_base=base + first, flags=flags, sample_seed=SSEED, temp_moves=n_moves), n_moves, cnt).copy()
        assert b.mcts_stats().faults == 0
        ex.finalize(b)
        out = (plays, bytes(b.download()), snapshot(ex, cnt, n_moves, n))
        b.close(); ex.close()
        return out

    ref = run(0, G, 0)
    for flags in (abi.mcts_tune(slots=1), abi.mcts_tune(slots=4), abi.mcts_tune(slots=8), abi.mcts_tune(parts=1), abi.mcts_tune(parts=2)):
        got = run(0, G, flags)
        assert np.array_equal(got[0], ref[0]) and got[1] == ref[1], flags
        same(got[2], ref[2], flags)
    h = G // 2
    for first in (0, h):
        got = run(first, h, 0)
        assert np.array_equal(got[0], ref[0][:, first:first + h])
        assert got[1] == ref[1][first * C.sizeof(TaflState):(first + h) * C.sizeof(TaflState)]
        part = {f: (ref[2][f][first:first + h] if f == "lens" else ref[2][f][:, first:first + h]) for f in FIELDS + ("lens",)}
        same(got[2], part, ("half", first))


def test_episode_in_pieces():
    """3 runs of 4 moves with move_base 0 / 4 / 8 (and the matching sim_offset) into one examples object == one run of 12."""
    rules, fen, wb, n, lg, glg = _mk("brandubh7")
    G, sims, cap, temp = 2048, 40, 64, 6
    a, states = _start(glg, fen, G, BASE)
    ex1 = glg.new_examples(G, 12, K)
    p1 = _plays_words(a.selfplay_record(ex1, 12, sims, 1.0, SEED, cap, game_id_base=BASE, sample_seed=SSEED, temp_moves=temp), 12, G)
    ex1.finalize(a)
    b = _batch(glg, states, G)
    ex2 = glg.new_examples(G, 12, K)
    rows = []
    for done in (0, 4, 8):
        rows.append(_plays_words(b.selfplay_record(ex2, 4, sims, 1.0, SEED, cap, game_id_base=BASE, sim_offset=done * sims, sample_seed=SSEED,
                                                   temp_moves=temp, move_base=done), 4, G).copy())
        ex2.finalize(b)                                              # repeatable: games still going on keep z = 0, final = 0
    assert np.array_equal(np.concatenate(rows), p1)
    assert pu.states_equal(a.download(), b.download(), G)
    same(snapshot(ex2, G, 12, n), snapshot(ex1, G, 12, n))
    S = snapshot(ex1, G, 12, n)
    assert set(np.unique(S["fin"])) == {0, 1}                        # games ended inside the run, others go on
    ex2.clear()
    assert ex2.counts()[1] == 0
    # play_episodes: the same episode through the package's loop (runs of 4 moves, move_base and sim_offset continued, then finalize)
    from alphazeroforhnefatafl_amd import MCTSArgs, play_episodes
    c = _batch(glg, states, G)
    lens, total, over = play_episodes(c, ex2, MCTSArgs(numMCTSSims=sims, cpuct=1.0, seed=SEED, max_rollout_plies=cap, game_id_base=BASE), 12, 4,
                                      sample_seed=SSEED, temp_moves=temp)
    fa = a.download()
    assert pu.states_equal(fa, c.download(), G)
    assert np.array_equal(np.frombuffer(lens, np.uint32), S["lens"]) and total == int(S["lens"].sum())
    assert over == int((pu.state_field(fa, G, "status") != abi.ONGOING).sum()) and 0 < over < G
    same(snapshot(ex2, G, 12, n), S)
    # every game over at the start: nothing is run, nothing is recorded
    d = glg.new_batch(64)
    over_ids = np.flatnonzero(pu.state_field(fa, G, "status") != abi.ONGOING)
    d.upload(_sub_states(fa, [int(over_ids[i % over_ids.size]) for i in range(64)]))
    ex3 = glg.new_examples(64, 4, K)
    assert play_episodes(d, ex3, MCTSArgs(numMCTSSims=sims, seed=SEED, max_rollout_plies=cap), 4, 2)[1:] == (0, 64)
    for h in (a, b, c, d, ex1, ex2, ex3):
        h.close()


def test_capacity_is_bookkeeping():
    """max_moves below the run: later examples dropped and counted, earlier ones intact.  max_children = 4 with S = 40: overflow marks,
    overflowed > 0 with stats.faults == 0, games still finish, plays and states as with a large K, every other example untouched."""
    rules, fen, wb, n, lg, glg = _mk("brandubh7")
    G, sims, n_moves, cap = 2048, 40, 12, 64
    a, states = _start(glg, fen, G, BASE)
    exa = glg.new_examples(G, n_moves, K)
    pa = _plays_words(a.selfplay_record(exa, n_moves, sims, 1.0, SEED, cap, game_id_base=BASE, sample_seed=SSEED, temp_moves=5), n_moves, G)
    exa.finalize(a)
    fa, A = a.download(), snapshot(exa, G, n_moves, n)
    assert (exa.stats().dropped, exa.stats().overflowed) == (0, 0)
    for max_moves, kk in ((5, K), (n_moves, 4)):
        b = _batch(glg, states, G)
        ex = glg.new_examples(G, max_moves, kk)
        pb = _plays_words(b.selfplay_record(ex, n_moves, sims, 1.0, SEED, cap, game_id_base=BASE, sample_seed=SSEED, temp_moves=5), n_moves, G)
        assert b.mcts_stats().faults == 0
        ex.finalize(b)
        assert np.array_equal(pa, pb) and pu.states_equal(fa, b.download(), G)
        B, es = snapshot(ex, G, max_moves, n), ex.stats()
        assert np.array_equal(B["lens"], np.minimum(A["lens"], max_moves))
        assert es.dropped == int((A["lens"] - B["lens"]).sum()) and (es.dropped > 0) == (max_moves < n_moves)
        wide = A["nc"][:max_moves] > kk
        assert es.overflowed == int(wide.sum()) and (es.overflowed > 0) == (kk == 4)
        assert np.array_equal(B["overflow"], wide.astype(np.uint8)) and not B["nc"][wide].any()
        for f in ("played", "move_no", "boards", "sides", "z", "fin"):
            assert np.array_equal(B[f], A[f][:max_moves]), f
        keep = ~wide
        assert np.array_equal(B["nc"][keep], A["nc"][:max_moves][keep])
        assert np.array_equal(B["acts"][keep][:, :kk], A["acts"][:max_moves][keep][:, :kk]) and np.array_equal(B["vis"][keep][:, :kk], A["vis"][:max_moves][keep][:, :kk])
        if wide.any():
            j, g = np.argwhere(wide)[0]
            _, _, pi, _, _ = ex.gather([j * G + g])
            assert not pi.any()
        b.close(); ex.close()
    # an examples object of another size is refused
    from alphazeroforhnefatafl_amd._lib import TaflError
    small = glg.new_examples(G // 2, 4, 8)
    with pytest.raises(TaflError) as ei:
        a.selfplay_record(small, 2, sims, 1.0, SEED, cap)
    assert ei.value.code == -1
    with pytest.raises(TaflError):
        small.gather([0])                                            # no example recorded: host pointers fail the call
    for h in (a, exa, small):
        h.close()


def test_gather_device_equals_host_equals_numpy():
    """65 536 rows, random indices and symmetries: device pointers into torch tensors == host pointers, and == numpy built from the
    oracle loop's examples for the rows of the spot ids under all eight symmetries; a row's float64 sum is within n_children * 2^-25 of 1."""
    import torch
    rules, fen, wb, n, lg, glg = _mk("copenhagen11")
    G, sims, n_moves, cap = 4096, 32, 5, 160
    a, states = _start(glg, fen, G, BASE)
    ex = glg.new_examples(G, n_moves, K)
    a.selfplay_record(ex, n_moves, sims, 1.0, SEED, cap, game_id_base=BASE, sample_seed=SSEED, temp_moves=n_moves, want_plays=False)
    ex.finalize(a)
    lens = np.frombuffer(ex.counts()[0], np.uint32)
    ids = [0, 63, 64, 2047, 2048, 4095, 1234, 7]
    sub = _sub_states(states, ids)
    _, o_ex, _ = xu.oracle_record(orc, lg, sub, len(ids), wb, sims, cap, 1.0, SEED, BASE, n_moves, SSEED, n_moves, 0, ids=[BASE + g for g in ids])
    spot = [(j, g, s, o_ex[i][j]) for i, g in enumerate(ids) for j in range(len(o_ex[i])) for s in range(8)]
    rng = np.random.default_rng(4)
    R = 65536
    gg = rng.integers(0, G, R)
    jj = (rng.integers(0, 1 << 30, R) % np.maximum(lens[gg], 1)).astype(np.int64)
    ok = lens[gg] > 0
    gg, jj = gg[ok], jj[ok]
    idx = np.concatenate([np.array([j * G + g for j, g, _, _ in spot], np.int64), jj * G + gg])[:R].astype(np.uint32)
    sym = np.concatenate([np.array([s for _, _, s, _ in spot], np.uint8), rng.integers(0, 8, gg.size).astype(np.uint8)])[:R]
    assert idx.size == R
    host = ex.gather(idx, sym)
    dev = ex.gather(torch.from_numpy(idx.view(np.int32)).cuda(), torch.from_numpy(sym).cuda(), device=True)
    for h, d, name in zip(host, dev, ("boards", "sides", "pi", "z", "final")):
        assert d.is_cuda and np.array_equal(h, d.cpu().numpy()), name
    ident = ex.gather(idx[:4096])                                    # sym = NULL: identity
    zero = ex.gather(idx[:4096], np.zeros(4096, np.uint8))
    for x, y in zip(ident, zero):
        assert np.array_equal(x, y)
    boards, sides, pi, z, fin = host
    for i, (j, g, s, e) in enumerate(spot):
        row = xu.dense_pi(n, e, s)
        assert np.array_equal(pi[i], row), (j, g, s)
        assert abs(float(row.astype(np.float64).sum()) - 1.0) <= len(e.actions) * 2.0 ** -25
        assert np.array_equal(boards[i], xu.sym_board_np(np.array(e.board, np.uint8), s)), (j, g, s)
        assert (sides[i], z[i], fin[i]) == (e.side, e.z, e.final)
    # every row against an expectation built without the gather kernel: the sparse (action, Nsa) of tafl_examples_read, the symmetry
    # tables of the Python restatement, float32(float64(Nsa) / float64(N)).  (The host-pointer gather launches chunks of at most 8 192 rows
    # = the grid's cap, one row per workgroup; the 65 536-row device launch sends every workgroup through 8 rows, so host == device also
    # holds the clearing of the LDS row between two rows against the single-row path.)
    A = abi.action_size(n)
    perm = np.array([[xu.sym_action_py(n, a_, s_) for a_ in range(A)] for s_ in range(8)])
    nc, ov, pl, mv, acts, vis = ex.read(idx)
    assert not ov.any() and (nc > 0).all()
    used = np.arange(K)[None, :] < nc[:, None]
    Nsum = np.where(used, vis, 0).sum(axis=1).astype(np.float64)
    rr, kk = np.nonzero(used)
    want_pi = np.zeros((R, A), np.float32)
    want_pi[rr, perm[sym[rr], acts[rr, kk]]] = (vis[rr, kk].astype(np.float64) / Nsum[rr]).astype(np.float32)
    if not np.array_equal(pi, want_pi):
        i = int(np.flatnonzero((pi != want_pi).any(axis=1))[0])
        raise AssertionError(("gather row", i, int(idx[i]), int(sym[i])))
    del want_pi
    tperm = np.array([[xu.sym_rc(n, t // n, t % n, s_)[0] * n + xu.sym_rc(n, t // n, t % n, s_)[1] for t in range(n * n)] for s_ in range(8)])
    b0 = _gather_no_pi(ex, idx)[0].reshape(R, n * n)                  # identity boards of the same examples
    want_b = np.zeros_like(b0)
    want_b[np.arange(R)[:, None], tperm[sym]] = b0
    assert np.array_equal(boards.reshape(R, n * n), want_b)
    sums = pi.astype(np.float64).sum(axis=1)
    assert np.abs(sums - 1.0).max() <= K * 2.0 ** -25
    assert (np.count_nonzero(pi, axis=1) <= K).all()
    # device pointers: an index that names no example gives an all-zero row and is counted
    bad = torch.tensor([int(lens[5]) * G + 5, n_moves * G + 9, int(idx[0])], dtype=torch.int32).cuda()
    b2, s2, p2, z2, f2 = ex.gather(bad, None, device=True)
    assert not b2[:2].any() and not p2[:2].any() and not s2[:2].any() and not z2[:2].any() and not f2[:2].any()
    assert np.array_equal(p2[2].cpu().numpy(), pi[0] if sym[0] == 0 else xu.dense_pi(n, spot[0][3], 0))
    assert ex.stats().bad_index == 2
    a.close(); ex.close()


def test_full_size_run_at_the_bench_settings():
    """65 536 Copenhagen 11x11 games from the start position, S = 64, cap 512, seed 2, 8 moves, all drawn (temp_moves = 8), K = 64:
    sims == G * 64 * 8, no fault, len all 8, and 4 oracle spot ids on both sides of the partition boundary."""
    rules, fen, wb, n, lg, glg = _mk("copenhagen11")
    G, sims, cap, seed, n_moves = 65536, 64, 512, 2, 8
    b = glg.new_batch(G, fen)
    ex = glg.new_examples(G, n_moves, 64)
    plays = _plays_words(b.selfplay_record(ex, n_moves, sims, 1.0, seed, cap, game_id_base=0, sample_seed=SSEED, temp_moves=8), n_moves, G)
    st = b.mcts_stats()
    assert st.sims == G * sims * n_moves and st.faults == 0
    ex.finalize(b)
    lens, total = ex.counts()
    assert total == G * n_moves and set(lens) == {n_moves}
    es = ex.stats()
    assert (es.dropped, es.overflowed) == (0, 0)
    (g0, g1), = pu.search_partitions(G, 2)[:1]
    ids = [0, g1 - 1, g1, G - 1]
    start = pu.start_states(orc, fen, rules.starting_side, wb, len(ids))
    o_plays, o_ex, info = xu.oracle_record(orc, lg, start, len(ids), wb, sims, cap, 1.0, seed, 0, n_moves, SSEED, 8, 0, ids=ids)
    assert info["widest"] < 64
    idx = np.array([j * G + g for g in ids for j in range(n_moves)], np.uint32)
    nc, ov, pl, mv, acts, vis = ex.read(idx)
    boards, sides, pi, z, fin = ex.gather(idx)
    fb = b.download()
    for i, g in enumerate(ids):
        assert bytes(start[i]) == bytes(fb[g]), g
        for j, e in enumerate(o_ex[i]):
            r, k = i * n_moves + j, len(e.actions)
            got = (boards[r].tolist(), int(sides[r]), acts[r, :k].tolist(), vis[r, :k].tolist(), int(pl[r]), int(mv[r]))
            assert int(nc[r]) == k and ov[r] == 0 and got == e.fields(), (g, j)
            assert np.array_equal(pi[r], xu.dense_pi(n, e)) and z[r] == e.z and fin[r] == e.final
        for m in range(n_moves):
            assert _word_tuple(plays[m, g]) == o_plays[m][i], (g, m)
    b.close(); ex.close()


def test_finalize_outcomes_including_a_draw():
    """k_examples_finalize for every result a game can have: states with the status set by hand to ongoing / attacker wins / defender wins
    / draw are uploaded behind a short run: z = 0, +1 / -1 from the example's side to move, 1e-4 for the draw; final."""
    rules, fen, wb, n, lg, glg = _mk("brandubh7")
    G, sims, cap = 256, 16, 64
    b = glg.new_batch(G, fen)
    ex = glg.new_examples(G, 3, K)
    b.selfplay_record(ex, 3, sims, 1.0, SEED, cap, want_plays=False)
    st = b.download()
    for g in range(G):
        st[g].status, st[g].winner = (abi.ONGOING, 1, 1, 2)[g % 4], (0, abi.ATTACKER, abi.DEFENDER, 0)[g % 4]
    b.upload(st)
    ex.finalize(b)
    S = snapshot(ex, G, 3, n)
    assert (S["lens"] == 3).all()
    for g in range(G):
        for j in range(3):
            assert (S["z"][j, g], S["fin"][j, g]) == xu.z_of(st[g], int(S["sides"][j, g])), (g, j)
    assert set(np.unique(S["z"]).tolist()) == {0.0, 1.0, -1.0, float(np.float32(1e-4))}
    b.close(); ex.close()
