"""Training examples of a recording self-play run (include/taflhip.h tafl_selfplay_record), CPU only: the product's
per-game functions (selfplay_pick, selfplay_advance_rec, example_outcome, sym_tile, sym_action) compiled for the host
(tests/hostsim/hostsim_examples.cpp) against the oracle loop and the Python restatements of tests/examples_util.py.  The same
comparisons run against the real kernels in tests/test_gpu_examples.py."""
import ctypes as C
import random

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflMctsParams
from oracle import oracle as orc
from tests import examples_util as xu
from tests import parity_util as pu
from tests.hostsim.hostsim import HostSim


def _mk(name):
    rules, fen, wb = pu.CONFIGS[name]
    n = abi.fen_side_len(fen)
    return rules, fen, wb, n, orc.GameLogic(rules, n)


def test_pick_is_the_cumulative_rule():
    """selfplay_pick == the rule of the header restated in Python: random visit vectors (1 .. 200 children, counts 1 .. 1000) x r at
    EVERY boundary ceil(j * 2^32 / N), j = 1 .. N, and one below it (the rule evaluated with np.cumsum + np.searchsorted, itself tied
    to the scalar restatement xu.pick_rule) x 1 000 random r; and for a fixed vector the pick frequencies over the 2^16 values
    r = i << 16 are the counts' proportions within 1 (exact arithmetic)."""
    L = xu.hlib()
    rng = random.Random(5)
    P32 = C.POINTER(C.c_uint32)
    for trial in range(60):
        m = rng.randrange(1, 201)
        vs = [rng.randrange(1, 1001) for _ in range(m)]
        N = sum(vs)
        j = np.arange(1, N + 1, dtype=np.uint64)
        bound = ((j << np.uint64(32)) + np.uint64(N - 1)) // np.uint64(N)       # ceil(j * 2^32 / N): the smallest r with (r * N) >> 32 >= j
        assert int(bound[-1]) == 1 << 32 and int(bound[0]) == -((-1 << 32) // N)
        rand = np.array([0, xu.M32] + [rng.randrange(1 << 32) for _ in range(1000)], np.uint64)
        rs = np.concatenate([np.minimum(bound, np.uint64(xu.M32)), bound - np.uint64(1), rand])
        k = (rs * np.uint64(N)) >> np.uint64(32)
        want = np.searchsorted(np.cumsum(np.array(vs, np.uint64)), k, side="right")       # the first child whose running sum exceeds k
        # every boundary between two children is among them: r = bound[s - 1] is the first word that picks the next child
        run = np.cumsum(vs)[:-1]
        if run.size:
            assert np.array_equal(want[run - 1], np.arange(1, m)) and np.array_equal(want[N + run - 1], np.arange(0, m - 1))
        for i in list(range(0, rs.size, max(1, rs.size // 500))) + list(range(rs.size - 1002, rs.size)):      # the vector form == the scalar restatement
            assert want[i] == xu.pick_rule(vs, int(rs[i])), (trial, int(rs[i]))
        arr, ra, out = (C.c_uint32 * m)(*vs), np.ascontiguousarray(rs, np.uint32), np.zeros(rs.size, np.uint32)
        L.hsx_pick_many(arr, m, ra.ctypes.data_as(P32), rs.size, out.ctypes.data_as(P32))
        if not np.array_equal(out, want):
            i = int(np.flatnonzero(out != want)[0])
            raise AssertionError((trial, int(rs[i]), int(out[i]), int(want[i])))
        assert L.hsx_pick(arr, m, int(rs[0])) == out[0]
    vs = [3, 1, 7, 2, 11, 5, 1, 9]
    N = sum(vs)
    rs = [i << 16 for i in range(1 << 16)]
    arr, ra, out = (C.c_uint32 * len(vs))(*vs), (C.c_uint32 * len(rs))(*rs), (C.c_uint32 * len(rs))()
    L.hsx_pick_many(arr, len(vs), ra, len(rs), out)
    freq = np.bincount(np.frombuffer(out, np.uint32), minlength=len(vs))
    for j, v in enumerate(vs):
        assert abs(int(freq[j]) - v * 65536 / N) <= 1, (j, freq[j], v * 65536 / N)
    # the word a move is drawn with: ply_rand(sim_key(game_key(sample_seed, gid), M), 0)
    for _ in range(200):
        s, g, mv = rng.randrange(1 << 64), rng.randrange(1 << 40), rng.randrange(1 << 20)
        assert L.hsx_rand(s, g, mv) == xu.sample_word(s, g, mv)


# (name, G, sims, n_moves, slots, target, capacity, advance modulus, sample_seed): the four settings of
# test_selfplay_run_equals_the_loop_of_searches_and_plays, a longer Brandubh run in which games end, and one with games over at the start
SETTINGS = [("brandubh7", 24, 40, 9, 8, 4, 0, 36, 11), ("copenhagen11", 8, 24, 4, 8, 4, 20, 36, 11), ("tablut9", 10, 30, 5, 4, 2, 0, 36, 11),
            ("copenhagen13", 4, 16, 3, 8, 4, 0, 36, 11), ("brandubh7", 24, 40, 12, 8, 4, 0, 36, 5), ("brandubh7", 24, 40, 12, 8, 4, 0, 60, 5)]
CAP, SEED, BASE = 60, 8, 50


def _start(name, G, mod):
    rules, fen, wb, n, lg = _mk(name)
    states = pu.start_states(orc, fen, rules.starting_side, wb, G)
    plies = (C.c_uint32 * G)(*[(i * 7) % mod for i in range(G)])
    orc.batch_random_advance(lg, states, G, wb, 3, plies, BASE)
    return rules, wb, n, lg, states


def _host_record(name, rules, n, wb, states, G, sims, n_moves, spec, sample_seed, temp_moves, move_base, max_moves=None, K=64):
    hx = xu.HostExamples(rules, n, wb, G, max_moves or n_moves, K)
    xu.hlib().hsx_set_dense13(int(name == "copenhagen13"))
    try:
        plays, stats = hx.record(states, TaflMctsParams(sims, CAP, 1.0, SEED, 0, 0), n_moves, BASE, sample_seed, temp_moves, move_base, spec)
    finally:
        xu.hlib().hsx_set_dense13(0)
    return hx, plays, stats


@pytest.mark.parametrize("idx", range(len(SETTINGS)))
def test_recording_run_equals_the_oracle_loop(idx):
    """Plays, final states, every field of every example, len and z after finalize == the oracle loop of tests/examples_util.py, with
    temp_moves = 0, 3 and n_moves and two move_base values.  The conditions that keep the comparison honest are asserted on the oracle
    loop alone: a quarter of all game-moves of a fully sampled run differ from the argmax, both sides to move occur, no root reaches
    n_sims visited children; in the fifth setting games end inside the run while others go on, in the sixth some are over at the start."""
    name, G, sims, n_moves, k, target, cap, mod, sseed = SETTINGS[idx]
    rules, wb, n, lg, states = _start(name, G, mod)
    over0 = sum(states[g].status != abi.ONGOING for g in range(G))
    cases = [(n_moves, 0)] if idx >= 4 else [(0, 0), (3, 0), (3, 2), (n_moves, 0), (n_moves + 2, 2)]
    for temp_moves, move_base in cases:
        want_states = pu.clone_states(states, G)
        want_plays, want_ex, info = xu.oracle_record(orc, lg, want_states, G, wb, sims, CAP, 1.0, SEED, BASE, n_moves, sseed, temp_moves, move_base)
        # -- honesty of the setting, from the oracle alone
        assert info["widest"] < sims, info
        assert {e.side for ex in want_ex for e in ex} == {abi.ATTACKER, abi.DEFENDER}
        if temp_moves >= move_base + n_moves:
            assert 4 * info["non_argmax"] >= info["game_moves"], info
        if temp_moves == 0:
            assert info["non_argmax"] == 0
        ended = sum(want_states[g].status != abi.ONGOING for g in range(G)) - over0
        if idx == 4:
            assert over0 == 0 and ended >= 2 and G - ended >= 2, (over0, ended)
            assert {e.final for ex in want_ex for e in ex} == {0, 1}
        if idx == 5:
            assert over0 == 4 and all(len(want_ex[g]) == 0 for g in range(G) if states[g].status != abi.ONGOING)
        # -- the harness
        got_states = pu.clone_states(states, G)
        hx, plays, stats = _host_record(name, rules, n, wb, got_states, G, sims, n_moves, (k, target, cap), sseed, temp_moves, move_base)
        where = (name, idx, temp_moves, move_base)
        for m in range(n_moves):
            assert [pu.play_tuple4(plays[m * G + g]) for g in range(G)] == want_plays[m], (where, m)
        assert pu.states_equal(want_states, got_states, G), (where, pu.first_state_diff(want_states, got_states, G))
        assert stats.faults == 0
        hx.finalize(got_states)
        lens, counters = hx.counts()
        assert counters == {"dropped": 0, "overflowed": 0, "bad_index": 0}
        xu.check_examples(hx.example, lens, want_ex, G, where)


@pytest.mark.parametrize("idx", range(4))
def test_temp_moves_zero_equals_selfplay_run(idx):
    """temp_moves == 0: the recording run's plays and final states are those of the existing self-play harness run (hs.selfplay), with
    and without an examples object."""
    from tests.hostsim import hostsim
    name, G, sims, n_moves, k, target, cap, mod, sseed = SETTINGS[idx]
    rules, wb, n, lg, states = _start(name, G, mod)
    hs = HostSim(rules, n, wb)
    hostsim.set_spec_k(k, target, cap)
    hostsim.set_dense13(name == "copenhagen13")
    try:
        a = pu.clone_states(states, G)
        want, _ = hs.selfplay(a, G, TaflMctsParams(sims, CAP, 1.0, SEED, 0, 0), n_moves, BASE)
    finally:
        hostsim.set_spec_k(4, 0, 0)
        hostsim.set_dense13(False)
    for record in (True, False):
        b = pu.clone_states(states, G)
        hx = xu.HostExamples(rules, n, wb, G, n_moves, 64)
        xu.hlib().hsx_set_dense13(int(name == "copenhagen13"))
        try:
            got, stats = hx.record(b, TaflMctsParams(sims, CAP, 1.0, SEED, 0, 0), n_moves, BASE, 99, 0, 0, (k, target, cap), record=record)
        finally:
            xu.hlib().hsx_set_dense13(0)
        assert bytes(got) == bytes(want), (name, record)
        assert pu.states_equal(a, b, G)
        assert (sum(hx.counts()[0]) > 0) == record


def test_capacity_is_bookkeeping():
    """max_moves below the run: later examples dropped and counted, earlier ones intact; max_children below the widest root: overflow marks,
    an all-zero gather row, the game goes on, plays and states unchanged, no other example disturbed."""
    name, G, sims, n_moves, k, target, cap, mod, sseed = SETTINGS[0]
    rules, wb, n, lg, states = _start(name, G, mod)
    want_states = pu.clone_states(states, G)
    want_plays, want_ex, info = xu.oracle_record(orc, lg, want_states, G, wb, sims, CAP, 1.0, SEED, BASE, n_moves, sseed, 3, 0)
    for max_moves, K in ((4, 64), (n_moves, 4)):
        got = pu.clone_states(states, G)
        hx, plays, stats = _host_record(name, rules, n, wb, got, G, sims, n_moves, (k, target, cap), sseed, 3, 0, max_moves, K)
        assert [[pu.play_tuple4(plays[m * G + g]) for g in range(G)] for m in range(n_moves)] == want_plays
        assert pu.states_equal(want_states, got, G) and stats.faults == 0
        hx.finalize(got)
        lens, counters = hx.counts()
        assert lens == [min(len(want_ex[g]), max_moves) for g in range(G)]
        assert counters["dropped"] == sum(max(0, len(want_ex[g]) - max_moves) for g in range(G))
        wide = sum(len(e.actions) > K for g in range(G) for e in want_ex[g])
        assert counters["overflowed"] == wide and (wide > 0) == (K == 4)
        for g in range(G):
            for j in range(lens[g]):
                e = want_ex[g][j]
                f, overflow, z, fin = hx.example(j, g)
                if len(e.actions) > K:
                    assert overflow == 1 and f == (e.board, e.side, [], [], e.played, e.move_no)
                    (_, _, pi, _, _), bad = hx.gather([j * G + g])
                    assert bad == 0 and not pi.any()
                else:
                    assert overflow == 0 and f == e.fields()
                assert z == e.z and fin == e.final


def test_symmetries():
    """(a) sym_tile / sym_action == the restatement from the header's formula for all actions x 8 on 7, 9, 11, 13; each is a bijection and
    the eight compose as the group does.  (b) tied to the rules: the oracle's legal mask of the transformed position == the transformed
    legal mask of the original, bit for bit, for 64 mid-game states per preset and all eight symmetries."""
    L = xu.hlib()
    for n in (7, 9, 11, 13):
        A = abi.action_size(n)
        tabs = []
        for k in range(8):
            tiles, acts = (C.c_uint32 * (n * n))(), (C.c_uint32 * A)()
            L.hsx_sym_tables(k, n, tiles, acts)
            tiles, acts = list(tiles), list(acts)
            assert tiles == [xu.sym_rc(n, t // n, t % n, k)[0] * n + xu.sym_rc(n, t // n, t % n, k)[1] for t in range(n * n)], (n, k)
            assert acts == [xu.sym_action_py(n, a, k) for a in range(A)], (n, k)
            assert sorted(acts) == list(range(A)) and sorted(tiles) == list(range(n * n))
            tabs.append((tiles, acts))
        tile_perms = [tuple(t) for t, _ in tabs]
        assert len(set(tile_perms)) == 8
        for a in range(8):
            for b in range(8):
                comp = tuple(tabs[b][0][tabs[a][0][t]] for t in range(n * n))        # a first, then b
                c = tile_perms.index(comp)                                          # closed: the composition is one of the eight
                assert [tabs[b][1][tabs[a][1][x]] for x in range(A)] == tabs[c][1], (n, a, b)
    for name in ("brandubh7", "tablut9", "copenhagen11", "copenhagen13"):
        rules, fen, wb, n, lg = _mk(name)
        G, A = 64, abi.action_size(n)
        states = pu.start_states(orc, fen, rules.starting_side, wb, G)
        plies = (C.c_uint32 * G)(*[(i * 5) % 40 + 1 for i in range(G)])
        orc.batch_random_advance(lg, states, G, wb, 21, plies, 0)
        live = [g for g in range(G) if states[g].status == abi.ONGOING]
        assert len(live) >= 32
        _, masks = orc.batch_movegen(lg, states, G, wb)
        mw = (A + 31) // 32
        base_bits = np.unpackbits(np.frombuffer(masks, np.uint8).reshape(G, mw * 4), axis=1, bitorder="little")[:, :A]
        for k in range(8):
            tr = (abi.TaflState * len(live))()
            for i, g in enumerate(live):
                cells = np.full((n, n), ".")
                for (r, c), ch in pu._fen_cells(abi.state_to_fen(states[g], wb)).items():
                    cells[r, c] = ch
                st = orc.GameState("/".join("".join(row) for row in _cells_to_fen_rows(xu.sym_board_np(cells, k))), states[g].side_to_play, wb).to_abi()
                C.memmove(C.byref(tr, i * C.sizeof(abi.TaflState)), C.byref(st), C.sizeof(abi.TaflState))
            _, tm = orc.batch_movegen(lg, tr, len(live), wb)
            tbits = np.unpackbits(np.frombuffer(tm, np.uint8).reshape(len(live), mw * 4), axis=1, bitorder="little")[:, :A]
            perm = np.array([xu.sym_action_py(n, a, k) for a in range(A)])
            for i, g in enumerate(live):
                want = np.zeros(A, np.uint8)
                want[perm] = base_bits[g]
                assert np.array_equal(tbits[i], want), (name, k, g)


def _cells_to_fen_rows(cells):
    """rows of single-character cells ('.' empty) -> FEN rows with run lengths of empty tiles."""
    rows = []
    for row in cells:
        out, run = [], 0
        for ch in row:
            if ch == ".":
                run += 1
            else:
                if run:
                    out.append(str(run)); run = 0
                out.append(ch)
        if run:
            out.append(str(run))
        rows.append(out)
    return rows


def test_gather_rows():
    """The harness gather == numpy built from the oracle loop's examples: float32(float64(Nsa) / float64(N)) at sigma(action), zeros
    elsewhere, a row's float64 sum within n_children * 2^-25 of 1; boards transformed with .T, flipud, fliplr; sides, z, final copied; an index
    beyond a game's len gives an all-zero row and is counted."""
    name, G, sims, n_moves, k, target, cap, mod, sseed = SETTINGS[4]
    rules, wb, n, lg, states = _start(name, G, mod)
    want_states = pu.clone_states(states, G)
    _, want_ex, _ = xu.oracle_record(orc, lg, want_states, G, wb, sims, CAP, 1.0, SEED, BASE, n_moves, sseed, n_moves, 0)
    got = pu.clone_states(states, G)
    hx, _, _ = _host_record(name, rules, n, wb, got, G, sims, n_moves, (k, target, cap), sseed, n_moves, 0)
    hx.finalize(got)
    rng = random.Random(3)
    pairs = [(j, g) for g in range(G) for j in range(len(want_ex[g]))]
    pick = [rng.choice(pairs) for _ in range(400)] + pairs[:8]
    syms = [rng.randrange(8) for _ in pick]
    for use_sym in (True, False):
        (boards, sides, pi, z, fin), bad = hx.gather([j * G + g for j, g in pick], syms if use_sym else None)
        assert bad == 0
        for i, (j, g) in enumerate(pick):
            e, s = want_ex[g][j], syms[i] if use_sym else 0
            row = xu.dense_pi(n, e, s)
            assert np.array_equal(pi[i], row), (i, j, g, s)
            assert abs(float(np.sum(row.astype(np.float64))) - 1.0) <= len(e.actions) * 2.0 ** -25
            assert np.array_equal(boards[i], xu.sym_board_np(np.array(e.board, np.uint8), s)), (i, s)
            assert (sides[i], z[i], fin[i]) == (e.side, e.z, e.final)
    short = next(g for g in range(G) if len(want_ex[g]) < n_moves)
    (boards, sides, pi, z, fin), bad = hx.gather([len(want_ex[short]) * G + short, n_moves * G + short, pick[0][0] * G + pick[0][1]])
    assert bad == 2 and not boards[:2].any() and not pi[:2].any() and not sides[:2].any() and not z[:2].any() and not fin[:2].any()
    assert np.array_equal(pi[2], xu.dense_pi(n, want_ex[pick[0][1]][pick[0][0]]))


def test_finalize_outcomes_including_a_draw():
    """example_outcome for every result a game can have: the recorded examples of a run, finalized against states whose status is set by
    hand to ongoing / attacker wins / defender wins / draw: z = 0, +1 / -1 from the example's side to move, TAFL_DRAW_VALUE; final."""
    name, G, sims, n_moves, k, target, cap, mod, sseed = SETTINGS[0]
    rules, wb, n, lg, states = _start(name, G, mod)
    got = pu.clone_states(states, G)
    hx, _, _ = _host_record(name, rules, n, wb, got, G, sims, 3, (k, target, cap), sseed, 0, 0, 3)
    lens, _ = hx.counts()
    for g in range(G):
        got[g].status, got[g].winner = (abi.ONGOING, 1, 1, 2)[g % 4], (0, abi.ATTACKER, abi.DEFENDER, 0)[g % 4]
    hx.finalize(got)
    seen = set()
    for g in range(G):
        for j in range(lens[g]):
            f, _, z, fin = hx.example(j, g)
            want = xu.z_of(got[g], f[1])
            assert (z, fin) == want, (g, j, z, fin, want)
            seen.add((float(z), fin))
    assert seen == {(0.0, 0), (1.0, 1), (-1.0, 1), (float(np.float32(1e-4)), 1)}
