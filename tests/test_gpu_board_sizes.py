"""The HIP kernels at every board size tafl_ctx_create accepts, through the C-ABI as tests/test_gpu_parity.py does, against the oracle on the
workloads of tests/board_sizes_util.py (proved on the CPU by tests/test_hostsim_board_sizes.py).  Bit-exact everywhere, no tolerances.

What only this file reaches: k_step<8, 15> / k_step_action<8, 15> (side 14 and 15; every other 256-bit batch steps
through the dense13 kernels), both sides of that boundary, the 8-limb layout without a padding column (15 @256) and with one (14 @256; also
10 @128 and 6 @64), even sides (throne on (n/2, n/2)), and the launches that depend on the side: k_select_kth / k_movegen_masks with 3 .. 6
and 14 / 15 waves per workgroup (960 threads, 55 KB of LDS at side 15) and masks of 2 and 3 words at side 3 and 4, where lines get an
empty chunk.  The coverage floors are asserted on the oracle's results before a kernel is compared.
"""
import ctypes as C
import random

import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflMctsParams, TaflPlay, TaflState
from oracle import oracle as orc
from tests import board_sizes_util as bu
from tests import guided_util as gu
from tests import parity_util as pu
from tests.board_sizes_util import gpu_batch, gpu_logic

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", range(3, 16))
def test_action_space_and_fen_through_the_context(n):
    """tafl_action_encode / tafl_action_decode over the whole action space, tafl_action_size / tafl_action_mask_words against n^2 * 2 (n - 1),
    tafl_state_from_fen / tafl_state_to_fen of start_fen(n) in every word that holds it (these take a context, which needs a device)."""
    from alphazeroforhnefatafl_amd._lib import lib
    L = lib()
    fen = bu.start_fen(n)
    for wb in (64, 128, 256):
        if n > abi.row_width(wb):
            continue
        lg = gpu_logic(abi.rules.COPENHAGEN, n, wb)
        A = n * n * 2 * (n - 1)
        assert lg.action_size == A == abi.action_size(n) and lg.mask_words == (A + 31) // 32
        if wb == abi.word_bits_for(n):
            for a in range(A):
                p, back = TaflPlay(), C.c_uint32()
                assert L.tafl_action_decode(lg._h, a, C.byref(p)) == 0 and L.tafl_action_encode(lg._h, p, C.byref(back)) == 0
                assert back.value == a and pu.play_tuple4(p) == pu.play_tuple4(abi.action_decode(n, a)), (n, a)
            assert L.tafl_action_decode(lg._h, A, C.byref(TaflPlay())) != 0
        st = lg.state_from_fen(fen, abi.ATTACKER)
        assert bytes(st) == bytes(orc.GameState(fen, abi.ATTACKER, wb).to_abi()), (n, wb)
        assert abi.state_to_fen(st, wb) == fen
        b = lg.new_batch(3, fen)
        assert all(bytes(s) == bytes(st) for s in b.download())
        b.close()


def _streamed(pair, label, rules, G, rng):
    n, wb = pair
    lg = orc.GameLogic(rules, n)
    tag = (pair, label, G)
    states = pu.random_board_states(rng, n, wb, G)
    b = gpu_batch(rules, n, wb, states, G)
    assert pu.states_equal(states, b.download(), G), tag
    oc, om = orc.batch_movegen(lg, states, G, wb)
    gc, gm = b.iter_plays()
    assert list(oc) == list(gc), tag
    assert bytes(om) == bytes(gm), tag
    gc2, _ = b.iter_plays(want_masks=False)
    assert list(oc) == list(gc2), tag
    plays = pu.random_plays(rng, n, G)
    codes = b.validate_play(plays)
    for g in range(G):
        assert lg.validate_play(plays[g], orc.GameState.from_abi(states[g], wb)) == codes[g], (tag, g, pu.describe_state(states[g], wb), pu.play_tuple4(plays[g]))
    for side in (abi.ATTACKER, abi.DEFENDER):
        out = b.side_can_play(side)
        for g in range(0, G, 3):
            assert lg.side_can_play(side, orc.GameState.from_abi(states[g], wb)) == bool(out[g]), (tag, g, side)
    enc = b.encode_boards()
    for g in range(0, G, 7):
        want = orc.GameState.from_abi(states[g], wb).board_to_matrix()
        assert [list(enc[g * n * n + r * n:g * n * n + (r + 1) * n]) for r in range(n)] == want, (tag, g)
    a = pu.clone_states(states, G)
    oe = orc.batch_step(lg, a, G, wb, plays)
    ge = b.do_play(plays)
    for g in range(G):
        assert pu.effects_tuple(oe[g]) == pu.effects_tuple(ge[g]), (tag, g)
    got = b.download()
    assert pu.states_equal(a, got, G), (tag, pu.first_state_diff(a, got, G))          # rejected plays leave the state untouched
    assert sum(1 for g in range(G) if oe[g].code != 0) > 0
    b.close()


@pytest.mark.parametrize("pair", bu.ALL_PAIRS, ids=bu.pair_id)
def test_streamed_calls_at_every_pair(pair):
    """iter_plays, validate_play, side_can_play, do_play with arbitrary plays and encode_boards at all 27 pairs under four rulesets; batches
    of 37 (the g >= n guard inside the side-many waves of a workgroup), 150 and 197 games; legal plays through do_play (k_step) as well."""
    n, wb = pair
    rng = random.Random(100 * n + wb)
    for (label, rules), G in zip(bu.rulesets(pair), (37, 150, 197, 70)):
        _streamed(pair, label, rules, G, rng)
    # legal plays through do_play: the oracle's play of a rank, handed to k_step as a play (at 14 / 15 @256: k_step<8, 15>)
    for label, rules in bu.rulesets(pair)[:2]:
        G = 131
        lg = orc.GameLogic(rules, n)
        states = pu.random_board_states(rng, n, wb, G)
        ranks = (C.c_uint32 * G)(*[rng.randrange(1 << 30) for _ in range(G)])
        a = pu.clone_states(states, G)
        op, oe = orc.batch_step_kth(lg, a, G, wb, ranks)
        b = gpu_batch(rules, n, wb, states, G)
        ge = b.do_play(op)
        oe2 = orc.batch_step(lg, pu.clone_states(states, G), G, wb, op)
        for g in range(G):
            assert pu.effects_tuple(oe2[g]) == pu.effects_tuple(ge[g]), (pair, label, g)
        assert sum(1 for g in range(G) if oe2[g].code == 0) > G // 2
        got = b.download()
        assert pu.states_equal(a, got, G), (pair, label, pu.first_state_diff(a, got, G))
        b.close()
    # the throne plays under the five rulesets
    states, plays, G = bu.throne_workload(pair)
    for label in bu.RULE_LABELS + ("copenhagen_kingpass",):
        rules = bu.ruleset(pair, label)
        lg = orc.GameLogic(rules, n)
        b = gpu_batch(rules, n, wb, states, G)
        assert [lg.validate_play(plays[g], orc.GameState.from_abi(states[g], wb)) for g in range(G)] == list(b.validate_play(plays)), (pair, label)
        b.close()


@pytest.mark.parametrize("pair", bu.EDGE_PAIRS, ids=bu.pair_id)
def test_every_legal_play_at_the_edge_pairs(pair):
    """Every legal play of the random and crafted positions under each ruleset (k_select_kth + k_step_action: <8, 15> at 14 and 15 @256, dense13
    at 12 and 13), after the floors on the oracle's results."""
    n, wb = pair
    bu.check_floors(pair)
    for label, rules in bu.rulesets(pair):
        bu.expand_compare_gpu(rules, n, wb, bu.position_list(pair), (pair, label), oracle=bu.oracle_expansion(pair, label))


@pytest.mark.parametrize("pair", bu.EDGE_PAIRS, ids=bu.pair_id)
def test_lockstep_games_at_the_edge_pairs(pair):
    """130 games (two full workgroups and a ragged one) from start_fen(n): random_advance against the oracle's, then 60 step_kth plies with
    masks every 10 plies and states at the end."""
    n, wb = pair
    G, T = 130, 60
    for label, rules in bu.rulesets(pair):
        lg = orc.GameLogic(rules, n)
        rng = random.Random(1234 + n)
        states = pu.start_states(orc, bu.start_fen(n), rules.starting_side, wb, G)
        b = gpu_logic(rules, n, wb).new_batch(G, bu.start_fen(n))
        plies = (C.c_uint32 * G)(*[(3 * g) % max(2, 2 * n) for g in range(G)])
        orc.batch_random_advance(lg, states, G, wb, 7, plies, 40)
        b.random_advance(7, plies, 40)
        got = b.download()
        assert pu.states_equal(states, got, G), (pair, label, "random_advance", pu.first_state_diff(states, got, G))
        for t in range(T):
            if t % 10 == 0:
                oc, om = orc.batch_movegen(lg, states, G, wb)
                gc, gm = b.iter_plays()
                assert list(oc) == list(gc), (pair, label, t)
                assert bytes(om) == bytes(gm), (pair, label, t)
            ranks = (C.c_uint32 * G)(*[rng.randrange(1 << 30) for _ in range(G)])
            before = pu.clone_states(states, G) if t % 10 == 0 else states
            op, oe = orc.batch_step_kth(lg, states, G, wb, ranks)
            gp, ge = b.do_kth_play(ranks)
            if not (bytes(op) == bytes(gp) and bytes(oe) == bytes(ge)):
                bu.assert_same_plays_effects((pair, label, t), wb, before, op, oe, gp, ge, G)
        got = b.download()
        assert pu.states_equal(states, got, G), (pair, label, pu.first_state_diff(states, got, G))
        b.close()


def test_rollout_terminations_seen_by_the_oracle():
    hist = bu.rollout_reason_hist(((14, 256), (15, 256)))
    assert len(hist) >= 4, hist
    for pair in ((5, 64), (4, 64), (3, 64)):
        h = bu.rollout_reason_hist((pair,))
        capped = sum(v for (_status, reason), v in h.items() if reason == abi.ROLLOUT_REASON_PLY_CAP)
        assert capped >= 10 and sum(h.values()) - capped >= 10, (pair, h)


@pytest.mark.parametrize("pair", bu.EDGE_PAIRS, ids=bu.pair_id)
def test_rollouts_at_the_edge_pairs(pair):
    """k_random_advance and k_rollout (the LDS index-to-mask tables; <8, 15, PRESET_NONE> at 12, 14, 15 @256) against the oracle's playouts:
    value, status, reason, winner and plies; the batch unchanged."""
    n, wb = pair
    G = bu.ROLLOUT_G
    for label, rules in bu.rulesets(pair):
        x = bu.rollout_expectation(pair, label)
        b = gpu_batch(rules, n, wb, x.before, G)
        b.random_advance(bu.ROLLOUT_ADVANCE_SEED, x.plies, bu.ROLLOUT_BASE)
        got = b.download()
        assert pu.states_equal(x.states, got, G), (pair, label, "random_advance", pu.first_state_diff(x.states, got, G))
        res = bu.result_tuples(b.rollout(bu.ROLLOUT_SEED, bu.ROLLOUT_SIM, bu.rollout_cap(n), bu.ROLLOUT_BASE), G)
        assert res == x.results, (pair, label, next(g for g in range(G) if res[g] != x.results[g]))
        assert pu.states_equal(x.states, b.download(), G), "tafl_rollout must not modify the batch"
        b.close()


def _pipelines(wb):
    if wb == 64:      # the fused kernel exists for 64-bit boards only (non-Brandubh rules: its run-time-rules instantiation)
        return (("default", 0), ("fused", abi.mcts_tune(abi.MCTS_PIPELINE_FUSED, 2)), ("two-kernel", abi.mcts_tune(abi.MCTS_PIPELINE_TWO_KERNEL, 4)))
    return (("default", 0),)


@pytest.mark.parametrize("s", bu.SEARCHES, ids=bu.search_id)
def test_searches_vs_oracle(s):
    """tafl_mcts_run against the oracle's root children (visits, q as hex), then mcts_play_best and the states."""
    n, wb = s.pair
    rules = bu.ruleset(s.pair, s.label)
    states, want, counts = bu.search_expectation(s)
    if n <= 5 or s.flags:
        assert s.sims > max(counts), (s, max(counts))
    sub = bu.best_plays(s)
    after = pu.clone_states(states, s.G)
    oeff = orc.batch_step(orc.GameLogic(rules, n), after, s.G, wb, sub)
    for label, tune in _pipelines(wb):
        b = gpu_batch(rules, n, wb, states, s.G)
        b.mcts_run(s.sims, bu.SEARCH_CPUCT, bu.SEARCH_SEED, s.cap, game_id_base=bu.SEARCH_BASE, flags=s.flags | tune)
        kids, cnt = b.mcts_root_children(bu.SEARCH_WIDTH)
        rec, cnt = pu.children_view(kids, cnt, s.G, bu.SEARCH_WIDTH)
        for g in range(s.G):
            assert pu.children_of(rec, cnt, g) == want[g], (bu.search_id(s), label, g)
        st = b.mcts_stats()
        assert st.sims == s.G * s.sims and st.faults == 0, (label, st.sims, st.faults)
        assert pu.states_equal(states, b.download(), s.G), "a search must not modify the batch"
        plays, eff = b.mcts_play_best()
        for g in range(s.G):
            if pu.play_tuple4(sub[g]) != (0, 0, 0, 0):
                assert pu.play_tuple4(plays[g]) == pu.play_tuple4(sub[g]), (bu.search_id(s), label, g)
                assert pu.effects_tuple(eff[g]) == pu.effects_tuple(oeff[g]), (bu.search_id(s), label, g)
            else:
                assert eff[g].code != 0
        got = b.download()
        assert pu.states_equal(after, got, s.G), (bu.search_id(s), label, pu.first_state_diff(after, got, s.G))
        b.close()


@pytest.mark.parametrize("pair", bu.GUIDED_PAIRS, ids=bu.pair_id)
def test_guided_search(pair):
    """tafl_gmcts_* with the stub evaluator against GameLogic.gmcts; at 15 @256 lane 0 is the crafted position with 328 legal plays:
    edges_per_node holds the widest root and no game faults."""
    n, wb = pair
    states, counts = bu.guided_workload(pair)
    assert max(counts) <= bu.guided_edges(pair), (pair, max(counts))
    if n == 15:
        assert counts[0] > 256
    want, want_counts = bu.guided_expectation(pair)
    b = gpu_batch(abi.rules.COPENHAGEN, n, wb, states, bu.GUIDED_G)
    kids, st, _ = gu.run_device_guided(b, bu.GUIDED_G, n, bu.GUIDED_SIMS, bu.GUIDED_CPUCT, bu.guided_salts(), bu.guided_edges(pair))
    for g in range(bu.GUIDED_G):
        assert kids[g] == want[g], (pair, g)
    assert (st.sims, st.predicts, st.terminal_hits) == want_counts and st.faults == 0, (st.sims, st.predicts, st.terminal_hits, st.faults, want_counts)
    b.close()


@pytest.mark.parametrize("pair,label,G,sims,n_moves,cap", [((15, 256), "copenhagen", 70, 12, 3, 48), ((8, 128), "brandubh", 70, 24, 3, 48)],
                         ids=["15@256-copenhagen", "8@128-brandubh"])
def test_selfplay_run_equals_the_synchronous_loop(pair, label, G, sims, n_moves, cap):
    """tafl_selfplay_run == the loop { tafl_mcts_run(sim_offset = move * n_sims); tafl_mcts_play_best }: plays of every move and final states,
    and one game against the same loop on the oracle."""
    n, wb = pair
    rules = bu.ruleset(pair, label)
    lg = orc.GameLogic(rules, n)
    states, _ = bu.advanced_start(pair, label, G, 2, 900, mod=max(2, 2 * n))
    a, b = gpu_batch(rules, n, wb, states, G), gpu_batch(rules, n, wb, states, G)
    want = []
    for m in range(n_moves):
        a.mcts_run(sims, 1.0, 6, cap, game_id_base=900, sim_offset=m * sims)
        plays, _ = a.mcts_play_best()
        want.append([pu.play_tuple4(plays[g]) for g in range(G)])
    got = b.selfplay_run(n_moves, sims, 1.0, 6, cap, game_id_base=900)
    for m in range(n_moves):
        assert [pu.play_tuple4(got[m * G + g]) for g in range(G)] == want[m], (pair, m)
    fa, fb = a.download(), b.download()
    assert pu.states_equal(fa, fb, G), pu.first_state_diff(fa, fb, G)
    assert b.mcts_stats().faults == 0
    g = 7
    one = (TaflState * 1)(states[g])
    for m in range(n_moves):
        kids, cnt, _ = orc.batch_mcts(lg, one, 1, wb, TaflMctsParams(sims, cap, 1.0, 6, m * sims, 0), 900 + g)
        vs = [kids[j].visits for j in range(cnt[0])]
        sub = (TaflPlay * 1)()
        if vs and max(vs) > 0 and one[0].status == 0:
            C.memmove(C.byref(sub[0]), C.byref(kids[vs.index(max(vs))].play), C.sizeof(TaflPlay))
        assert pu.play_tuple4(sub[0]) == want[m][g], (pair, m)
        orc.batch_step(lg, one, 1, wb, sub)
    assert bytes(one[0]) == bytes(fb[g])
    a.close(); b.close()
