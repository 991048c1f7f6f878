"""Every search variant `bench.py --full` publishes, at the benchmark's own settings (65 536 games, cap 512, seed 2, c_puct 1.0, game ids
from 0), against the CPU oracle and against a second route through the library.  The inputs are built with the recipe of bench.py's
run_variants (constants copied, bench.py is not imported).  Bit-exact everywhere: there is no tolerance in this file.

Per rollout-mode variant: the conservation laws of the step over ALL games, scattered ids (batch ends, wave boundary, both sides of every
stream-partition boundary) against oracle.batch_mcts, and all 65 536 games against the same search with one slot, no prediction and one
partition - the two routes share the rules engine but not the scheduling, prediction, partitioning or work-list code.  Brandubh: every
game against the oracle's digests (tests/golden/bench_brandubh7_S64.json).  Needs a real MI355X: `pytest -m gpu`."""
import ctypes as C
import json
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflMctsParams, TaflPlay, TaflState
from oracle import oracle as orc
from tests import parity_util as pu

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# bench.py: GAMES_PER_GPU, --seed, --max-plies, --cpuct defaults, BOARDS
GAMES_PER_GPU, SEED, CAP, CPUCT = 65536, 2, 512, 1.0
BOARDS = {"copenhagen11": ("COPENHAGEN", "COPENHAGEN", 11, 128), "copenhagen13": ("COPENHAGEN", "COPENHAGEN13", 13, 256),
          "brandubh7": ("BRANDUBH", "BRANDUBH", 7, 64)}
# max_children of the readers: the legal plays at the start position (116 at 11x11, 152 at 13x13); a search of S simulations visits at most
# S - 1 root children, which is what bounds the mixed positions and Brandubh at S = 64
WIDTH = {"copenhagen11": 116, "copenhagen13": 152, "brandubh7": 64}

# name -> (board, S, mixed positions, ids beyond pu.boundary_ids).  Mixed: ids advanced by 61 - 63 plies (from the start position the
# search is one level deep; from mid-game positions the oracle visits 1 - 4 root children to depth ~2: select and backup at work).
VARIANTS = {
    "mcts_S256": ("copenhagen11", 256, False, ()),
    "mcts_S1000": ("copenhagen11", 1000, False, ()),
    "mcts_mixed_positions_S64": ("copenhagen11", 64, True, (61, 126, 1983, 31999, 50047, 65470)),
    "mcts_13x13_S64": ("copenhagen13", 64, False, (4097,)),
    "mcts_brandubh7_S64": ("brandubh7", 64, False, tuple(range(1021, 65536, 1093))),
}


def _board(board):
    rn, bn, side, wb = BOARDS[board]
    return getattr(abi.rules, rn), getattr(abi.boards, bn), side, wb


def _gpu_logic(board):
    from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
    rules, _fen, side, wb = _board(board)
    return BatchedGameLogic(rules, side, wb, device=0)


def _is_fused_by_default(wb):
    """mcts_begin: with default tuning flags a 64-bit board is searched by k_mcts_fused (one stream, no partitions)."""
    return wb == 64


def variant_ids(name, G=GAMES_PER_GPU):
    board, _sims, _mixed, extra = VARIANTS[name]
    parts = pu.default_search_parts(G, _is_fused_by_default(BOARDS[board][3]))
    return sorted(set(pu.boundary_ids(G, parts)) | {i for i in extra if i < G})


def oracle_state(olg, board, mixed, gid):
    """The position of game `gid` under bench.py's recipe, computed by the oracle alone."""
    rules, fen, _side, wb = _board(board)
    st = orc.GameState(fen, rules.starting_side, wb)
    if mixed:
        st = olg.random_advance(st, 1, gid, gid % 64)
    return st.to_abi()


@pytest.mark.parametrize("name", list(VARIANTS))
def test_rollout_variant_at_bench_settings(name):
    """One variant of bench.py's run_variants on its 65 536-game batch (see the module docstring).  S = 256 and S = 1000 additionally
    have to BE the benchmarked machinery: predictions issued and hit, and - from the round trace of the first partition - more rounds
    with playouts than ceil(S / slots), i.e. slack or straggler rounds.  The library has no getter for the slot count of a default plan
    (slots = what the device holds at once / games); the test reads it off the trace: a round runs min(requested, the partition's share
    of the device) playouts, the games of a full round request more than that share (about six per game at four slots), so the largest
    `run` of the trace is the share and share // games of the partition is the plan's slot count."""
    board, sims, mixed, _extra = VARIANTS[name]
    rules, fen, side, wb = _board(board)
    G = GAMES_PER_GPU
    fused = _is_fused_by_default(wb)
    width = WIDTH[board]
    ids = variant_ids(name)
    assert {0, 63, 64, G - 1} <= set(ids)
    if not fused:
        assert {G // 2 - 1, G // 2} <= set(ids)                       # two partitions of 512 waves each

    olg = orc.GameLogic(rules, side)
    p = TaflMctsParams(sims, CAP, CPUCT, SEED, 0, 0)
    ostates = {g: oracle_state(olg, board, mixed, g) for g in ids}
    pool = ThreadPoolExecutor(max_workers=1)                          # the oracle works on the host while the GPU searches
    want_f = pool.submit(pu.oracle_children_parallel, orc, olg, wb, p, [(g, ostates[g], g) for g in ids], 256, 15)

    logic = _gpu_logic(board)
    batch = logic.new_batch(G, fen)
    if mixed:
        batch.random_advance(1, (C.c_uint32 * G)(*[i % 64 for i in range(G)]), 0)
    states = batch.download()
    for g in ids:
        assert bytes(states[g]) == bytes(ostates[g]), f"{name}: input position of game {g} differs from the oracle's"
    batch.mcts_reserve(sims)
    batch.mcts_run(sims, CPUCT, SEED, CAP, game_id_base=0)

    # 1. conservation
    st = batch.mcts_stats()
    print(f"{name}: sims {st.sims} rollouts {st.rollouts} terminal_hits {st.terminal_hits} faults {st.faults} spec {st.spec_hits}/{st.spec_issued} "
          f"capped {st.reason_hist[14]}")
    assert st.sims == G * sims and st.faults == 0
    assert st.rollouts + st.terminal_hits == st.sims and sum(st.reason_hist) == st.rollouts
    rec, cnt = pu.children_view(*batch.mcts_root_children(width), G, width)
    over = pu.state_field(states, G, "status") != abi.ONGOING
    if mixed:
        assert sorted(np.flatnonzero(over[:4096]).tolist()) == [503, 1070, 3000]
    else:
        assert not over.any()
    sums = pu.root_visit_sums(rec, cnt)
    bad = np.flatnonzero(sums != np.where(over, 0, sims - 1))
    assert bad.size == 0, f"{name}: root visits of game {int(bad[0])} sum to {int(sums[bad[0]])}"

    # 4. the benchmarked machinery
    if sims >= 256:
        assert st.spec_issued > 0 and st.spec_hits > 0
        req, run = batch.mcts_round_trace()
        g0, g1 = pu.search_partitions(G, pu.default_search_parts(G, fused))[0]
        slots = max(run) // (g1 - g0)
        active = sum(1 for r in run if r > 0)
        print(f"{name}: rounds enqueued {len(req)}, with playouts {active}, rounds 0..3 requested {req[:4]} run {run[:4]}, slots {slots}")
        assert 1 <= slots <= 8 and max(req) > max(run)                 # (some round was cut to the share: the share is what `run` shows)
        assert active > math.ceil(sims / slots), (active, slots)

    # 3. every game by a second route: one slot, no prediction, one partition (Brandubh: the two-kernel pipeline instead of k_mcts_fused)
    route2 = abi.mcts_tune(abi.MCTS_PIPELINE_TWO_KERNEL if fused else 0, 1, 1)
    first = {g: pu.children_of(rec, cnt, g) for g in ids}
    batch.mcts_run(sims, CPUCT, SEED, CAP, game_id_base=0, flags=route2)
    s2 = batch.mcts_stats()
    assert s2.sims == G * sims and s2.faults == 0
    rec2, cnt2 = pu.children_view(*batch.mcts_root_children(width), G, width)
    g = pu.first_children_diff(rec, cnt, rec2, cnt2)
    assert g < 0, f"{name}: game {g} differs between the default route and the one-slot route; entries of one side only: " \
                  f"{sorted(set(pu.children_of(rec, cnt, g)) ^ set(pu.children_of(rec2, cnt2, g)))}"
    for f in ("rollouts", "rollout_plies", "tree_depth_sum", "children_scanned", "terminal_hits"):
        assert getattr(st, f) == getattr(s2, f), (name, f)
    assert list(st.reason_hist) == list(s2.reason_hist)

    # Brandubh: every game against the oracle (digests of blocks of 64 games)
    if name == "mcts_brandubh7_S64":
        with open(os.path.join(HERE, "golden", "bench_brandubh7_S64.json")) as f:
            gold = json.load(f)
        assert (gold["games"], gold["sims"], gold["max_rollout_plies"], gold["seed"], gold["c_puct"], gold["block"]) == (G, sims, CAP, SEED, CPUCT, 64)
        got = pu.children_block_digests(rec, cnt, block=64)
        diff = [i for i in range(len(got)) if got[i] != gold["sha256"][i]]
        assert not diff, f"{name}: block {diff[0]} (games {diff[0] * 64} .. {diff[0] * 64 + 63}) differs from the oracle; {len(diff)} blocks differ"
    batch.close(); logic.close()

    # 2. oracle ids
    want = want_f.result()
    pool.shutdown()
    for g in ids:
        assert first[g] == want[g], f"{name}: game {g} differs from the oracle"
    if mixed:                                                          # the chosen ids do exercise select and backup below the root
        assert any(len(want[g]) and max(v for _a, v, _q in want[g]) > 1 for g in ids)


def _oracle_selfplay(olg, wb, state, gid, n_moves, sims):
    """The loop {search with sim_offset = m * sims; play the first most visited root child} on the oracle: (plays, final state)."""
    one = (TaflState * 1)(state)
    plays = []
    for m in range(n_moves):
        p = TaflMctsParams(sims, CAP, CPUCT, SEED, m * sims, 0)
        kids, cnt, _ = orc.batch_mcts(olg, one, 1, wb, p, gid)
        vs = [kids[j].visits for j in range(cnt[0])]
        sub = (TaflPlay * 1)()
        if vs and max(vs) > 0 and one[0].status == 0:
            C.memmove(C.byref(sub[0]), C.byref(kids[vs.index(max(vs))].play), C.sizeof(TaflPlay))
        plays.append(pu.play_tuple4(sub[0]))
        orc.batch_step(olg, one, 1, wb, sub)
    return plays, bytes(one[0])


def test_selfplay_run_at_bench_settings():
    """`selfplay_continuous_S64`: tafl_selfplay_run(8 moves, S = 64) on 65 536 11x11 games from the start position, as bench.py's
    selfplay_variant runs it (warm-up run of two moves, reset, the measured run).  sims == G * 64 * 8 and no faults; the plays of every
    move and the final states of ALL games equal the synchronous loop {mcts_run(sim_offset = m * 64); mcts_play_best} on a second batch;
    the batch ends and both sides of the partition boundary are replayed move by move on the oracle."""
    board, sims, n_moves, G = "copenhagen11", 64, 8, GAMES_PER_GPU
    rules, fen, side, wb = _board(board)
    olg = orc.GameLogic(rules, side)
    ids = pu.boundary_ids(G, pu.default_search_parts(G, False))
    start = oracle_state(olg, board, False, 0)
    pool = ThreadPoolExecutor(max_workers=min(15, len(ids)))
    want_f = {g: pool.submit(_oracle_selfplay, olg, wb, start, g, n_moves, sims) for g in ids}

    logic = _gpu_logic(board)
    a = logic.new_batch(G, fen)
    a.mcts_reserve(sims)
    a.selfplay_run(2, sims, CPUCT, SEED, CAP, want_plays=False)
    a.reset_fen(fen, rules.starting_side)
    got = a.selfplay_run(n_moves, sims, CPUCT, SEED, CAP)
    st = a.mcts_stats()
    assert st.faults == 0 and st.sims == G * sims * n_moves, (st.sims, st.faults)
    got = np.frombuffer(got, dtype="<u4").reshape(n_moves, G).copy()
    fa = a.download()
    a.close()

    b = logic.new_batch(G, fen)
    for m in range(n_moves):
        b.mcts_run(sims, CPUCT, SEED, CAP, game_id_base=0, sim_offset=m * sims)
        plays, _ = b.mcts_play_best()
        want_m = np.frombuffer(plays, dtype="<u4")
        bad = np.flatnonzero(want_m != got[m])
        assert bad.size == 0, f"move {m}: game {int(bad[0])} played differently in the self-play run; {bad.size} games differ"
    fb = b.download()
    assert pu.states_equal(fa, fb, G), pu.first_state_diff(fa, fb, G)
    b.close(); logic.close()

    for g in ids:
        oplays, ofinal = want_f[g].result()
        gplays = [pu.play_tuple4(TaflPlay.from_buffer_copy(got[m, g].tobytes())) for m in range(n_moves)]
        assert gplays == oplays, g
        assert bytes(fa[g]) == ofinal, g
    pool.shutdown()


# ---- guided_engine_only_S64 ----------------------------------------------------------------------------------------------------------

GUIDED_K = 64                                                          # rows of the evaluator's tables


def guided_tables(action_size, side):
    """An exact, position-dependent stand-in for nnet.predict that costs one gather: the position hashes to h = (sum(board_to_matrix *
    w) + 131 * side_to_play) mod K in integer arithmetic, priors = table[h], value = vtable[h].  The tables are built like
    tests/stub_net.py builds its outputs (24-bit mantissas scaled by powers of two, so that the float64 sum of a masked row rounds;
    values k / 2^20); every seventh row is all-zero (the "all valid moves were masked" branch, mcts.py:91-98)."""
    rs = np.random.RandomState(20240)
    w = rs.randint(1, 1000, size=side * side).astype(np.int64)
    mant = rs.randint(1 << 23, 1 << 24, size=(GUIDED_K, action_size)).astype(np.float32)
    expo = rs.randint(0, 40, size=(GUIDED_K, action_size))
    table = np.ldexp(mant, -24 - expo).astype(np.float32)
    table[::7] = 0
    vtable = (rs.randint(-(1 << 20), (1 << 20) + 1, size=GUIDED_K).astype(np.float32) / np.float32(1 << 20)).astype(np.float32)
    return w, table, vtable


def guided_hash(boards, sides, w):
    """boards int64 [n, side * side], sides int64 [n] -> row index [n] (numpy; the device evaluator does the same in torch)."""
    return ((boards * w[None, :]).sum(axis=1) + 131 * sides) % GUIDED_K


class _HostEval:
    """predict_batch through host buffers (numpy)."""

    def __init__(self, n, side, tables):
        self.n, self.nn, (self.w, self.table, self.vtable) = n, side * side, tables
        self.keep = None

    def predict_batch(self, boards, sides, waiting):
        b = np.frombuffer(boards, dtype=np.uint8).reshape(self.n, self.nn).astype(np.int64)
        h = guided_hash(b, np.frombuffer(sides, dtype=np.uint8).astype(np.int64), self.w)
        p, v = np.ascontiguousarray(self.table[h]), np.ascontiguousarray(self.vtable[h])
        self.keep = (p, v)
        return p.ctypes.data_as(C.POINTER(C.c_float)), v.ctypes.data_as(C.POINTER(C.c_float))


def _guided_children(batch, n, width=64):
    return pu.children_view(*batch.gmcts_root_children(width), n, width)


def test_guided_at_bench_settings():
    """`guided_engine_only_S64`: 65 536 11x11 games, S = 64, device pointers, edges_per_node = 192, as bench.py's guided_variant runs it -
    but on mixed positions (game i advanced by i mod 64 plies) and with an evaluator that depends on the position (guided_tables): the
    bench's constant evaluator would hide a wrong leaf board.  259 ids against oracle.gmcts with the same evaluator on the host;
    gmcts_stats; the first 8 192 games against a second batch driven through HOST pointers (whole buffers); and the oracle ids as a
    batch of their own, whose `predicts` must equal the oracle's count."""
    import torch
    from alphazeroforhnefatafl_amd.mcts import GuidedMCTS, MCTSArgs
    board, sims, G, H, epn = "copenhagen11", 64, GAMES_PER_GPU, 8192, 192
    rules, fen, side, wb = _board(board)
    logic = _gpu_logic(board)
    A = logic.action_size
    tables = guided_tables(A, side)
    w, table, vtable = tables
    assert not table[0].any() and table[1].all()
    dev = torch.device("cuda:0")
    args = MCTSArgs(numMCTSSims=sims, cpuct=CPUCT)

    b = logic.new_batch(G, fen)
    b.random_advance(1, (C.c_uint32 * G)(*[i % 64 for i in range(G)]), 0)
    states = b.download()

    class DeviceEval:
        def __init__(self):
            self.boards = torch.zeros((G, side, side), dtype=torch.uint8, device=dev)
            self.sides = torch.zeros(G, dtype=torch.uint8, device=dev)
            self.waiting = torch.zeros(G, dtype=torch.uint8, device=dev)
            self.w = torch.from_numpy(w).to(dev)
            self.table, self.vtable = torch.from_numpy(table).to(dev), torch.from_numpy(vtable).to(dev)
            self.pri = torch.zeros((G, A), dtype=torch.float32, device=dev)      # persistent outputs
            self.val = torch.zeros(G, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()

        def predict_batch(self, *_ptrs):
            h = ((self.boards.view(G, -1).to(torch.int64) * self.w).sum(1) + 131 * self.sides.to(torch.int64)) % GUIDED_K
            torch.index_select(self.table, 0, h, out=self.pri)
            torch.index_select(self.vtable, 0, h, out=self.val)
            torch.cuda.synchronize()
            return self.pri.data_ptr(), self.val.data_ptr()

    net = DeviceEval()
    m = GuidedMCTS(b, net, args, edges_per_node=epn, device=True, buffers=(net.boards.data_ptr(), net.sides.data_ptr(), net.waiting.data_ptr()))
    m.search_all()
    gs = b.gmcts_stats()
    print(f"guided: rounds {m.rounds} sims {gs.sims} predicts {gs.predicts} terminal_hits {gs.terminal_hits} faults {gs.faults}")
    assert gs.sims == G * sims and gs.faults == 0 and gs.waiting == 0
    assert gs.predicts > 0 and gs.predicts + gs.terminal_hits == gs.sims      # every search ends in predict() or in a finished game
    rec, cnt = _guided_children(b, G)
    b.close()
    del net, m
    torch.cuda.empty_cache()
    over = pu.state_field(states, G, "status") != abi.ONGOING
    sums = pu.root_visit_sums(rec, cnt)
    bad = np.flatnonzero(sums != np.where(over, 0, sims - 1))
    assert bad.size == 0, f"guided: root visits of game {int(bad[0])} sum to {int(sums[bad[0]])}"

    # the first 8 192 games through host pointers
    hb = logic.new_batch(H)
    hb.upload((TaflState * H).from_buffer_copy(bytes(states)[:H * C.sizeof(TaflState)]))
    hm = GuidedMCTS(hb, _HostEval(H, side, tables), args, edges_per_node=epn)
    hm.search_all()
    hs = hb.gmcts_stats()
    assert hs.sims == H * sims and hs.faults == 0
    hrec, hcnt = _guided_children(hb, H)
    g = pu.first_children_diff(rec[:H], cnt[:H], hrec, hcnt)
    assert g < 0, f"guided: game {g} differs between device pointers (65 536 games) and host pointers (8 192 games): " \
                  f"{pu.children_of(rec, cnt, g)} != {pu.children_of(hrec, hcnt, g)}"
    hb.close()

    # oracle ids
    ids = sorted({0, 63, 64, G - 1} | set(range(37, G, 257)))
    assert len(ids) >= 256
    olg = orc.GameLogic(rules, side)

    def predict(s):
        mtx = np.array(s.board_to_matrix(), dtype=np.int64).reshape(1, -1)
        h = int(guided_hash(mtx, np.array([int(s.side_to_play)], dtype=np.int64), w)[0])
        return table[h], vtable[h]

    want, want_predicts, deep = {}, 0, 0
    for gid in ids:
        ost = olg.random_advance(orc.GameState(fen, rules.starting_side, wb), 1, gid, gid % 64)
        assert bytes(ost.to_abi()) == bytes(states[gid]), gid
        kids, _ns, _pri, counts = olg.gmcts(ost, sims, CPUCT, predict, wb)
        want[gid] = [(a, v, float(q).hex()) for (_p, a, v, q) in kids]
        want_predicts += counts[1]
        deep += bool(kids) and max(v for (_p, _a, v, _q) in kids) > 1
    for gid in ids:
        assert pu.children_of(rec, cnt, gid) == want[gid], f"guided: game {gid} differs from the oracle"
    assert deep > len(ids) // 2                                        # the trees are not flat
    # the same ids as a batch of their own: the statistics the oracle can speak about
    n = len(ids)
    sb = logic.new_batch(n)
    sb.upload((TaflState * n)(*[states[gid] for gid in ids]))
    sm = GuidedMCTS(sb, _HostEval(n, side, tables), args, edges_per_node=epn)
    sm.search_all()
    ss = sb.gmcts_stats()
    assert (ss.sims, ss.predicts, ss.faults) == (n * sims, want_predicts, 0)
    srec, scnt = _guided_children(sb, n)
    for i, gid in enumerate(ids):
        assert pu.children_of(srec, scnt, i) == want[gid], gid
    sb.close(); logic.close()
