"""GPU parity tests: the HIP kernels, called through the C-ABI (include/taflhip.h), against the CPU oracle
on identical seeded inputs, the committed golden fixtures (reference KATs, reference-mcts.py vectors) and
size-independent properties at BASELINE.json's full batch size.  Bit-exact everywhere (integer / index work;
float64 Qsa compared as bit patterns).  Needs a real MI355X: `pytest -m gpu`.
"""
import collections
import ctypes as C
import json
import os
import random

import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflMctsParams, TaflPlay, TaflState
from oracle import oracle as orc
from tests import parity_util as pu
from tests.board_sizes_util import expand_compare_gpu as _expand_compare_gpu, gpu_batch, gpu_logic    # (shared with tests/test_gpu_board_sizes.py)
from tests.kat_util import KATS, REASON_CODE, play, ruleset, side_of, status_tuple, tiles

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _mk(name):
    rules, fen, wb = pu.CONFIGS[name]
    n = abi.fen_side_len(fen)
    return rules, fen, wb, n, orc.GameLogic(rules, n)


def test_native_library_is_loaded():
    """The HIP extension (in-tree libtaflhip.so) must be the thing that runs: no silent fallback exists."""
    from alphazeroforhnefatafl_amd import _lib
    L = _lib.lib()
    assert os.path.basename(_lib.LIB_PATH) == "libtaflhip.so" and os.path.exists(_lib.LIB_PATH)
    with open("/proc/self/maps") as f:
        assert "libtaflhip.so" in f.read()
    assert L.tafl_abi_version() == abi.ABI_VERSION
    lg = gpu_logic(abi.rules.COPENHAGEN, 11, 128)
    assert lg.action_size == 2420 and lg.mask_words == 76


def test_upload_download_roundtrip_and_fen():
    rng = random.Random(3)
    for n, wb in ((7, 64), (11, 128), (9, 128), (13, 256)):
        states = pu.random_board_states(rng, n, wb, 300)
        b = gpu_batch(abi.rules.COPENHAGEN, n, wb, states, 300)
        back = b.download()
        assert pu.states_equal(states, back, 300), (n, wb)
    for name, (rules, fen, wb) in pu.CONFIGS.items():
        n = abi.fen_side_len(fen)
        lg = gpu_logic(rules, n, wb)
        b = lg.new_batch(70, fen)
        got = b.download()
        want = orc.GameState(fen, rules.starting_side, wb).to_abi()
        for g in (0, 33, 69):
            assert bytes(got[g]) == bytes(want), name
        assert bytes(lg.state_from_fen(fen)) == bytes(want), name


def test_config2_movegen_and_step_4096_copenhagen():
    """BASELINE.json configs[1]: batch 4096 11x11 Copenhagen games, move-gen + step kernels, bit-exact vs CPU."""
    rules, fen, wb, n, lg = _mk("copenhagen11")
    G = 4096
    glg = gpu_logic(rules, n, wb)
    b = glg.new_batch(G, fen)
    plies = (C.c_uint32 * G)(*[i % 64 for i in range(G)])
    b.random_advance(1, plies, 0)
    ostates = pu.start_states(orc, fen, rules.starting_side, wb, G)
    orc.batch_random_advance(lg, ostates, G, wb, 1, plies, 0)
    gstates = b.download()
    assert pu.states_equal(ostates, gstates, G), pu.first_state_diff(ostates, gstates, G)
    rng = random.Random(5)
    for t in range(6):
        oc, om = orc.batch_movegen(lg, ostates, G, wb)
        gc, gm = b.iter_plays()
        assert list(oc) == list(gc), t
        assert bytes(om) == bytes(gm), t
        ranks = (C.c_uint32 * G)(*[rng.randrange(1 << 30) for _ in range(G)])
        op, oe = orc.batch_step_kth(lg, ostates, G, wb, ranks)
        gp, ge = b.do_kth_play(ranks)
        for g in range(G):
            assert pu.play_tuple4(op[g]) == pu.play_tuple4(gp[g]), (t, g)
            assert pu.effects_tuple(oe[g]) == pu.effects_tuple(ge[g]), (t, g)
        gstates = b.download()
        assert pu.states_equal(ostates, gstates, G), (t, pu.first_state_diff(ostates, gstates, G))


@pytest.mark.parametrize("name", list(pu.CONFIGS))
def test_lockstep_games(name):
    rules, fen, wb, n, lg = _mk(name)
    G, T = 192, 120
    rng = random.Random(1234)
    states = pu.start_states(orc, fen, rules.starting_side, wb, G)
    b = gpu_batch(rules, n, wb, states, G)
    for t in range(T):
        if t % 10 == 0:
            oc, om = orc.batch_movegen(lg, states, G, wb)
            gc, gm = b.iter_plays()
            assert list(oc) == list(gc), (name, t)
            assert bytes(om) == bytes(gm), (name, t)
        ranks = (C.c_uint32 * G)(*[rng.randrange(1 << 30) for _ in range(G)])
        op, oe = orc.batch_step_kth(lg, states, G, wb, ranks)
        gp, ge = b.do_kth_play(ranks)
        for g in range(G):
            assert pu.play_tuple4(op[g]) == pu.play_tuple4(gp[g]), (name, t, g)
            assert pu.effects_tuple(oe[g]) == pu.effects_tuple(ge[g]), (name, t, g)
        if t % 10 == 9 or t == T - 1:
            got = b.download()
            assert pu.states_equal(states, got, G), (name, t, pu.first_state_diff(states, got, G))


def test_rare_rules_crafted_positions():
    """Enclosure win, exit fort, shieldwall, sparse endgames: every legal play of crafted positions."""
    rng = random.Random(21)
    C11 = abi.rules.COPENHAGEN
    cov = collections.Counter()
    for n, wb in ((11, 128), (13, 256), (9, 128)):
        cov += _expand_compare_gpu(C11, n, wb, pu.enclosure_positions(rng, n, wb, 150), ("encl", n))
        cov += _expand_compare_gpu(C11, n, wb, pu.exit_fort_positions(rng, n, wb, 150), ("fort", n))
        cov += _expand_compare_gpu(C11, n, wb, pu.shieldwall_positions(rng, n, wb, 200), ("sw", n))
        cov += _expand_compare_gpu(C11, n, wb, pu.sparse_endgame_positions(rng, n, wb, 150), ("sparse", n))
    cov += _expand_compare_gpu(abi.rules.BRANDUBH, 7, 64, pu.enclosure_positions(rng, 7, 64, 150), ("encl", 7))
    cov += _expand_compare_gpu(abi.rules.BRANDUBH, 7, 64, pu.sparse_endgame_positions(rng, 7, 64, 200), ("sparse", 7))
    cov += _expand_compare_gpu(abi.rules.TABLUT, 9, 128, pu.sparse_endgame_positions(rng, 9, 128, 200), ("sparse-tablut", 9))
    dense = pu.random_board_states(rng, 11, 128, 400, density=0.7)
    cov += _expand_compare_gpu(C11, 11, 128, [dense[i] for i in range(400)], ("dense", 11))
    assert cov[(abi.WIN, abi.ENCLOSED)] >= 20, cov
    assert cov[(abi.WIN, abi.EXIT_FORT)] >= 50, cov
    assert cov[(abi.WIN, abi.KING_CAPTURED)] >= 10, cov
    assert cov[(abi.WIN, abi.ALL_CAPTURED)] >= 1, cov


@pytest.mark.parametrize("seed", range(10))
def test_random_rulesets(seed):
    rng = random.Random(2000 + seed)
    rules = pu.random_ruleset(rng)
    n, wb = rng.choice([(7, 64), (9, 128), (11, 128), (13, 256)])
    lst = [s for s in pu.random_board_states(rng, n, wb, 100)] + pu.enclosure_positions(rng, n, wb, 30) + \
        pu.shieldwall_positions(rng, n, wb, 40) + pu.sparse_endgame_positions(rng, n, wb, 40)
    if n >= 9:
        lst += pu.exit_fort_positions(rng, n, wb, 30)
    _expand_compare_gpu(rules, n, wb, lst, ("fuzz", seed))
    # validate codes for arbitrary plays
    G = len(lst)
    states = pu.states_array(lst)
    plays = pu.random_plays(rng, n, G)
    b = gpu_batch(rules, n, wb, states, G)
    codes = b.validate_play(plays)
    lg = orc.GameLogic(rules, n)
    for g in range(G):
        st = orc.GameState.from_abi(states[g], wb)
        assert lg.validate_play(plays[g], st) == codes[g], (seed, g)
    for side in (abi.ATTACKER, abi.DEFENDER):
        out = b.side_can_play(side)
        for g in range(0, G, 5):
            st = orc.GameState.from_abi(states[g], wb)
            assert lg.side_can_play(side, st) == bool(out[g]), (seed, g, side)
    # arbitrary plays through do_play (mostly rejected: state must stay untouched, code must match)
    a = pu.clone_states(states, G)
    oe = orc.batch_step(lg, a, G, wb, plays)
    ge = b.do_play(plays)
    for g in range(G):
        assert pu.effects_tuple(oe[g]) == pu.effects_tuple(ge[g]), (seed, g)
    assert pu.states_equal(a, b.download(), G)


@pytest.mark.parametrize("name,G,cap", [("copenhagen11", 1024, 512), ("brandubh7", 512, 256), ("tablut9", 512, 300),
                                       ("copenhagen13", 256, 300), ("magpie7", 256, 200),
                                       # the 256-bit word WITHOUT the dense 13-column preset layout: k_rollout<8,15,8,15,0>
                                       ("copenhagen9_u256", 256, 300), ("tablut13_u256", 192, 300)])
def test_rollouts(name, G, cap):
    rules, fen, wb, n, lg = _mk(name)
    states = pu.start_states(orc, fen, rules.starting_side, wb, G)
    plies = (C.c_uint32 * G)(*[(i * 7) % 50 for i in range(G)])
    orc.batch_random_advance(lg, states, G, wb, 3, plies, 500)
    b = gpu_batch(rules, n, wb, states, G)
    ro = orc.batch_rollout(lg, states, G, wb, 5, 9, cap, 500)
    rg = b.rollout(5, 9, cap, 500)
    for g in range(G):
        assert (ro[g].value, ro[g].status, ro[g].reason, ro[g].winner, ro[g].plies) == \
               (rg[g].value, rg[g].status, rg[g].reason, rg[g].winner, rg[g].plies), (name, g)
    assert pu.states_equal(states, b.download(), G), "tafl_rollout must not modify the batch"


def test_kat_replay_through_the_c_abi():
    """The reference's own unit tests (tests/golden/reference_kats.json) replayed on the GPU path."""
    # test_iter_plays (game/game/mod.rs:137-207): legal sets per piece from the dense mask
    for case in KATS["iter_plays"]["cases"]:
        rules = ruleset(case["rules"])
        lg = gpu_logic(rules, 7, case["word_bits"])
        for side in (abi.ATTACKER, abi.DEFENDER):
            b = lg.new_batch(1, case["fen"], side)
            _, masks = b.iter_plays()
            acts = [a for a in range(lg.action_size) if (masks[a >> 5] >> (a & 31)) & 1]
            per_tile = collections.defaultdict(set)
            for a in acts:
                p = abi.action_decode(7, a)
                per_tile[(p.from_row, p.from_col)].add(abi.play_to(p))
            st = orc.GameState(case["fen"], side, case["word_bits"])
            for q in case["queries"]:
                pc = st.get_piece(tuple(q["tile"]))
                if q["expected"] is None or pc is None or pc[1] != side:
                    continue
                assert per_tile[tuple(q["tile"])] == tiles(q["expected"]), q
    # test_play_validity (logic.rs:923-1013) on 64/128/256-bit words
    for wb in (64, 128, 256):
        b = None
        rules = None
        for step in KATS["play_validity"]["script"]:
            op = step["op"]
            if op == "new":
                rules = ruleset(step["rules"])
                b = gpu_logic(rules, 7, wb).new_batch(1, step["fen"], side_of(step["side"], rules))
            elif op in ("valid", "invalid"):
                code = b.validate_play((TaflPlay * 1)(play(step["play"])))[0]
                assert code == (0 if op == "valid" else REASON_CODE[step["reason"]]), (wb, step)
            elif op == "do_play":
                eff = b.do_play((TaflPlay * 1)(play(step["play"])))
                assert eff[0].code == 0
            elif op == "board_move":
                st = orc.GameState.from_abi(b.download()[0], wb)
                st.move_piece(tuple(step["from"]), tuple(step["to"]))
                b.upload((TaflState * 1)(st.to_abi()))
            elif op == "set_side":
                st = b.download()
                st[0].side_to_play = abi.ATTACKER if step["side"] == "A" else abi.DEFENDER
                b.upload(st)
    # test_play_outcome (logic.rs:1023-1079)
    k = KATS["play_outcome"]
    rules = ruleset(k["rules"])
    for wb in (64, 128, 256):
        for case in k["cases"]:
            b = gpu_logic(rules, 7, wb).new_batch(1, k["fen"], side_of(case["side"], rules))
            eff = b.do_play((TaflPlay * 1)(play(case["play"])))[0]
            assert eff.code == 0 and (eff.status, eff.reason, eff.winner) == status_tuple(case["status"]), (wb, case)
            assert _caps(eff, abi.row_width(wb)) == tiles(case["captures"]), (wb, case)
    # test_strong_king_capture (logic.rs:1424-1462), test_linnaean_capture (:1465-1482)
    k = KATS["strong_king_capture"]
    for case in k["cases"]:
        b = gpu_logic(ruleset(k["rules"]), 7, 64).new_batch(1, case["fen"], abi.ATTACKER)
        eff = b.do_play((TaflPlay * 1)(play(case["play"])))[0]
        assert _caps(eff, 7) == tiles(case["captures"]) and (eff.status, eff.reason, eff.winner) == status_tuple(case["outcome"]), case
    k = KATS["linnaean_capture"]
    b = gpu_logic(ruleset(k["rules"]), 9, 128).new_batch(1, k["fen"], abi.ATTACKER)
    eff = b.do_play((TaflPlay * 1)(play(k["play"])))[0]
    assert _caps(eff, 11) == tiles(k["captures"])
    # test_repetitions (logic.rs:1406-1421)
    k = KATS["repetitions"]
    b = gpu_logic(ruleset(k["rules"]), 7, 64).new_batch(1, k["fen"], abi.ATTACKER)
    for _ in range(k["cycles"]):
        for s in k["cycle"]:
            assert b.do_play((TaflPlay * 1)(abi.play_from_str(s)))[0].code == 0
    st = b.download()[0]
    assert (st.status, st.reason, st.winner) == status_tuple(k["status_after_cycles"])
    eff = b.do_play((TaflPlay * 1)(abi.play_from_str(k["final_play"])))[0]
    assert (eff.status, eff.reason, eff.winner) == status_tuple(k["final_status"])
    # test_can_play (logic.rs:1388-1403), derived opening counts
    k = KATS["can_play"]
    for case in k["cases"]:
        b = gpu_logic(ruleset(k["rules"]), 7, 64).new_batch(1, case["fen"], abi.ATTACKER)
        assert bool(b.side_can_play(abi.ATTACKER)[0]) == case["attacker"]
        assert bool(b.side_can_play(abi.DEFENDER)[0]) == case["defender"]
    for case in KATS["derived_counts"]["cases"]:
        n = abi.fen_side_len(case["fen"])
        b = gpu_logic(ruleset(case["rules"]), n, abi.word_bits_for(n)).new_batch(3, case["fen"], abi.ATTACKER if case["side"] == "A" else abi.DEFENDER)
        counts, _ = b.iter_plays(want_masks=False)
        assert list(counts) == [case["count"]] * 3
    # exit forts / shieldwalls (logic.rs:1090-1233) through do_play equivalence with the oracle are in the crafted tests


def _caps(eff, rw):
    out = set()
    for limb in range(abi.MAX_LIMBS):
        v = int(eff.captures[limb])
        while v:
            bpos = (v & -v).bit_length() - 1
            bit = limb * 64 + bpos
            out.add((bit // rw, bit % rw))
            v &= v - 1
    return out


with open(os.path.join(HERE, "golden", "mcts_golden.json")) as f:
    GOLD = json.load(f)


@pytest.mark.parametrize("case", GOLD["cases"], ids=[c["name"] for c in GOLD["cases"]])
def test_mcts_matches_reference_mcts_py_golden(case):
    """Root statistics produced by the reference's src/mcts.py (tests/golden/make_mcts_golden.py) reproduced on the GPU."""
    rules = abi.rules.BY_NAME[case["rules"]]
    st = TaflState.from_buffer_copy(bytes.fromhex(case["state_hex"]))
    G = 3                                  # the golden game plus two decoys with other ids in the same wave
    arr = (TaflState * G)(st, st, st)
    b = gpu_batch(rules, case["side_len"], case["word_bits"], arr, G)
    # decoys get ids game_id+1, +2; the golden game is game 0 with base = game_id
    b.mcts_run(case["n_sims"], case["cpuct"], case["seed"], case["max_plies"], game_id_base=case["game_id"])
    kids, cnt = b.mcts_root_children(256)
    got = [[kids[j].action, kids[j].visits, float(kids[j].q).hex()] for j in range(cnt[0])]
    assert got == case["root_children"]
    stats = b.mcts_stats()
    assert stats.sims == G * case["n_sims"] and stats.faults == 0
    # policy of mcts.py:48-53 at temp = 1
    probs = b.mcts_policy(1.0)
    nz = [(a, float(probs[a]).hex()) for a in range(b.logic.action_size) if probs[a] != 0]
    assert nz == [tuple(x) for x in case["probs_temp1_nonzero"]]
    assert pu.states_equal(arr, b.download(), G), "tafl_mcts_run must not modify the batch"


@pytest.mark.parametrize("name,G,sims,cpuct,cap", [("copenhagen11", 64, 64, 1.0, 512), ("brandubh7", 128, 200, 1.0, 256),
                                                  ("tablut9", 64, 96, 1.5, 300), ("copenhagen13", 32, 32, 1.0, 256),
                                                  ("copenhagen13", 6, 190, 1.0, 48), ("copenhagen11", 6, 400, 1.0, 48),
                                                  # run-time-rules kernels of the 256-bit word: k_mcts_tree / k_mcts_rollout<8,15,0>
                                                  ("copenhagen9_u256", 32, 48, 1.0, 200), ("tablut13_u256", 16, 32, 1.0, 200),
                                                  # c_puct == 0: an unvisited action TIES a visited one with Qsa == 0 (mcts.py:117-119)
                                                  ("brandubh7", 64, 200, 0.0, 256), ("copenhagen11", 16, 120, 0.0, 64),
                                                  # mixed mid-game positions (the config-1 input recipe) at the bench's S = 64 / cap 512
                                                  ("copenhagen11:mid", 48, 64, 1.0, 512)])
def test_mcts_vs_oracle(name, G, sims, cpuct, cap):
    """BASELINE config 3 parity: a fixed subset of games reproduced by the CPU oracle bit for bit.  (The two long searches: a root that
    grows past the 128 edges whose Qsa signs the tree step caches - 13x13 has 152 legal plays at the start - and deep trees.)"""
    name, _, variant = name.partition(":")
    rules, fen, wb, n, lg = _mk(name)
    states = pu.start_states(orc, fen, rules.starting_side, wb, G)
    if variant == "mid":
        plies = (C.c_uint32 * G)(*[(i * 7 + 3) % 64 for i in range(G)])
        orc.batch_random_advance(lg, states, G, wb, 1, plies, 77)
    elif name != "copenhagen11":
        plies = (C.c_uint32 * G)(*[(i * 5) % 40 for i in range(G)])
        orc.batch_random_advance(lg, states, G, wb, 11, plies, 77)
    p = TaflMctsParams(sims, cap, cpuct, 2, 0, 0)
    ok, on, ostats = orc.batch_mcts(lg, states, G, wb, p, 77)
    b = gpu_batch(rules, n, wb, states, G)
    b.mcts_run(sims, cpuct, 2, cap, game_id_base=77)
    gk, gn = b.mcts_root_children(256)
    assert list(on) == list(gn)
    for g in range(G):
        for j in range(on[g]):
            x, y = ok[g * 256 + j], gk[g * 256 + j]
            assert (pu.play_tuple4(x.play), x.action, x.visits, float(x.q).hex()) == \
                   (pu.play_tuple4(y.play), y.action, y.visits, float(y.q).hex()), (name, g, j)
    gs = b.mcts_stats()
    for f in ("sims", "rollouts", "rollout_plies", "tree_depth_sum", "children_scanned", "terminal_hits", "faults"):
        assert getattr(ostats, f) == getattr(gs, f), f
    assert list(ostats.reason_hist) == list(gs.reason_hist)
    # best play / dense visits consistent with the children list
    bp, bv = b.mcts_best_play()
    dense = b.mcts_root_visits()
    for g in range(G):
        vs = [gk[g * 256 + j].visits for j in range(gn[g])]
        if not vs:                      # root already terminal: nothing was searched
            assert bv[g] == 0
            continue
        assert bv[g] == max(vs)
        assert pu.play_tuple4(bp[g]) == pu.play_tuple4(gk[g * 256 + vs.index(max(vs))].play)
        for j in range(gn[g]):
            assert dense[g * b.logic.action_size + gk[g * 256 + j].action] == gk[g * 256 + j].visits
        assert sum(dense[g * b.logic.action_size:(g + 1) * b.logic.action_size]) == sum(vs)


def test_full_size_properties_65536():
    """BASELINE full size (65 536 concurrent 11x11 games): sharding invariance (results depend on the GLOBAL game id
    only, so 1/2/4/8-GPU runs agree), oracle spot checks, and conservation properties."""
    rules, fen, wb, n, lg = _mk("copenhagen11")
    G = 65536
    glg = gpu_logic(rules, n, wb)
    big = glg.new_batch(G, fen)
    sims, cap, seed = 8, 128, 2
    big.mcts_run(sims, 1.0, seed, cap, game_id_base=0)
    kids, cnt = big.mcts_root_children(16)
    st = big.mcts_stats()
    assert st.sims == G * sims and st.faults == 0
    assert st.rollouts + st.terminal_hits == st.sims
    assert sum(st.reason_hist) == st.rollouts
    # every game: root visits sum to sims - 1 (the first simulation only expands the root, mcts.py:83-102)
    for g in range(0, G, 97):
        assert sum(kids[g * 16 + j].visits for j in range(cnt[g])) == sims - 1
    # shard invariance: the second half as its own batch with game_id_base = G/2
    half = glg.new_batch(G // 2, fen)
    half.mcts_run(sims, 1.0, seed, cap, game_id_base=G // 2)
    hk, hc = half.mcts_root_children(16)
    for g in range(0, G // 2, 61):
        a = [(kids[(G // 2 + g) * 16 + j].action, kids[(G // 2 + g) * 16 + j].visits, kids[(G // 2 + g) * 16 + j].q) for j in range(cnt[G // 2 + g])]
        bb = [(hk[g * 16 + j].action, hk[g * 16 + j].visits, hk[g * 16 + j].q) for j in range(hc[g])]
        assert a == bb, g
    # oracle spot check on scattered game ids
    ids = [0, 1, 63, 64, 4097, 32768, 65535]
    p = TaflMctsParams(sims, cap, 1.0, seed, 0, 0)
    one = pu.start_states(orc, fen, rules.starting_side, wb, 1)
    for gid in ids:
        ok, on, _ = orc.batch_mcts(lg, one, 1, wb, p, gid)
        want = [(ok[j].action, ok[j].visits, float(ok[j].q).hex()) for j in range(on[0])]
        got = [(kids[gid * 16 + j].action, kids[gid * 16 + j].visits, float(kids[gid * 16 + j].q).hex()) for j in range(cnt[gid])]
        assert want == got, gid
    # rollouts at full size: value/status consistency + oracle spot check
    res = big.rollout(7, 0, 512, 0)
    hist = collections.Counter()
    for g in range(0, G, 13):
        r = res[g]
        hist[r.reason] += 1
        assert r.plies <= 512
        if r.status == abi.WIN:
            assert r.value in (-1, 1) and (r.value == 1) == (r.winner == abi.ATTACKER)
        else:
            assert r.value == 0
    oneres = orc.batch_rollout(lg, one, 1, wb, 7, 0, 512, 4097)
    assert (oneres[0].value, oneres[0].reason, oneres[0].plies) == (res[4097].value, res[4097].reason, res[4097].plies)
    assert pu.states_equal(pu.start_states(orc, fen, rules.starting_side, wb, 64), big.download(0, 64), 64)


def _kids(kids, cnt, g, width):
    return [(kids[g * width + j].action, kids[g * width + j].visits, float(kids[g * width + j].q).hex()) for j in range(cnt[g])]


def _oracle_kids(lg, state, wb, p, gid):
    one = (TaflState * 1)(state)
    ok, on, _ = orc.batch_mcts(lg, one, 1, wb, p, gid)
    return [(ok[j].action, ok[j].visits, float(ok[j].q).hex()) for j in range(on[0])]


def test_long_search_with_device_side_width_control_vs_oracle():
    """S = 300 at four slots per game is planned for 75 rounds (>= 64): the width cap of the prediction pass is then steered on the device
    from the hit rate of the last 16 rounds (k_mcts_rollout, CT_WCAP), two partitions run on two streams, and the stragglers' rounds are
    run by tafl_mcts_wait.  8 192 games from mixed mid-game positions; scattered ids against the oracle, all counters conserved."""
    rules, fen, wb, n, lg = _mk("copenhagen11")
    G, sims, cap, seed, base = 8192, 300, 96, 9, 1000
    b = gpu_logic(rules, n, wb).new_batch(G, fen)
    plies = (C.c_uint32 * G)(*[i % 64 for i in range(G)])
    b.random_advance(1, plies, base)
    states = b.download()
    b.mcts_run(sims, 1.0, seed, cap, game_id_base=base, flags=abi.mcts_tune(0, 4, 2))
    st = b.mcts_stats()
    assert st.sims == G * sims and st.faults == 0 and st.rollouts + st.terminal_hits == st.sims
    assert st.spec_issued > 0 and st.spec_hits > 0
    kids, cnt = b.mcts_root_children(256)
    p = TaflMctsParams(sims, cap, 1.0, seed, 0, 0)
    for gid in (0, 63, 64, 1777, 4095, 4096, 8191):
        assert _kids(kids, cnt, gid, 256) == _oracle_kids(lg, states[gid], wb, p, base + gid), gid
    # the same search with one slot (no prediction at all) must agree game by game
    b.mcts_run(sims, 1.0, seed, cap, game_id_base=base, flags=abi.mcts_tune(0, 1, 1))
    k1, c1 = b.mcts_root_children(256)
    for g in range(0, G, 37):
        assert _kids(kids, cnt, g, 256) == _kids(k1, c1, g, 256), g


def test_async_searches_equal_the_synchronous_one_and_the_oracle():
    """tafl_mcts_run_async / _after / tafl_mcts_wait: two half-size batches searched side by side, the second half a search behind the first,
    re-issued several times like a self-play loop - per game identical to one synchronous search of the whole id range and to the oracle."""
    rules, fen, wb, n, lg = _mk("copenhagen11")
    G, H, sims, cap, seed = 16384, 8192, 40, 160, 4
    glg = gpu_logic(rules, n, wb)
    whole = glg.new_batch(G, fen)
    plies = (C.c_uint32 * G)(*[(i * 3) % 48 for i in range(G)])
    whole.random_advance(1, plies, 0)
    states = whole.download()
    whole.mcts_run(sims, 1.0, seed, cap, game_id_base=0)
    wk, wc = whole.mcts_root_children(64)
    halves = [glg.new_batch(H), glg.new_batch(H)]
    for i, hb in enumerate(halves):
        hb.upload((TaflState * H).from_buffer_copy(bytes(states)[i * H * C.sizeof(TaflState):(i + 1) * H * C.sizeof(TaflState)]))
    for rep in range(3):
        halves[0].mcts_run_async(sims, 1.0, seed, cap, game_id_base=0)
        halves[1].mcts_run_async(sims, 1.0, seed, cap, game_id_base=H, after=halves[0])
        if rep == 1:                                     # re-issue the first while the second is still in flight
            halves[0].mcts_wait()
            halves[0].mcts_run_async(sims, 1.0, seed, cap, game_id_base=0)
        for hb in halves:
            hb.mcts_wait()
    for i, hb in enumerate(halves):
        st = hb.mcts_stats()
        assert st.sims == H * sims and st.faults == 0
        hk, hc = hb.mcts_root_children(64)              # (a reader joins a search in flight by itself; here it is already joined)
        for g in range(0, H, 29):
            assert _kids(hk, hc, g, 64) == _kids(wk, wc, i * H + g, 64), (i, g)
    p = TaflMctsParams(sims, cap, 1.0, seed, 0, 0)
    hk, hc = halves[1].mcts_root_children(64)
    for g in (0, 77, 8191):
        assert _kids(hk, hc, g, 64) == _oracle_kids(lg, states[H + g], wb, p, H + g), g
    # a reader called without tafl_mcts_wait joins the search itself
    halves[0].mcts_run_async(sims, 1.0, seed, cap, game_id_base=0)
    k2, c2 = halves[0].mcts_root_children(64)
    for g in range(0, H, 411):
        assert _kids(k2, c2, g, 64) == _kids(wk, wc, g, 64), g
    assert pu.states_equal(states, whole.download(), 64), "searches must not modify the batch"


@pytest.mark.parametrize("name,G,sims,n_moves,cap", [("copenhagen11", 4096, 32, 5, 160), ("brandubh7", 2048, 40, 12, 64), ("copenhagen13", 512, 16, 3, 96)])
def test_selfplay_run_equals_the_synchronous_loop(name, G, sims, n_moves, cap):
    """tafl_selfplay_run (every game searches and plays at its own pace, k_mcts_tree_selfplay) == the loop
    { tafl_mcts_run(sim_offset = move * n_sims); tafl_mcts_play_best } on the same batch: plays of every move and final states, including
    games that end on the way (Brandubh: many do) and the 13x13 preset (search in the dense layout, plays applied to the 15-column batch)."""
    rules, fen, wb, n, lg = _mk(name)
    glg = gpu_logic(rules, n, wb)
    a = glg.new_batch(G, fen)
    plies = (C.c_uint32 * G)(*[(i * 5) % 30 for i in range(G)])
    a.random_advance(2, plies, 900)
    states = a.download()
    b = gpu_batch(rules, n, wb, states, G)
    want = []
    for m in range(n_moves):
        a.mcts_run(sims, 1.0, 6, cap, game_id_base=900, sim_offset=m * sims)
        plays, _ = a.mcts_play_best()
        want.append([pu.play_tuple4(plays[g]) for g in range(G)])
    got = b.selfplay_run(n_moves, sims, 1.0, 6, cap, game_id_base=900)
    for m in range(n_moves):
        assert [pu.play_tuple4(got[m * G + g]) for g in range(G)] == want[m], (name, m)
    fa, fb = a.download(), b.download()
    assert pu.states_equal(fa, fb, G), pu.first_state_diff(fa, fb, G)
    st = b.mcts_stats()
    assert st.faults == 0
    if name == "brandubh7":
        assert sum(1 for g in range(G) if fb[g].status != 0) > G // 20          # games did end on the way
    # oracle spot check of one game: the same loop on the CPU
    g = 7
    one = (TaflState * 1)(states[g])
    for m in range(n_moves):
        p = TaflMctsParams(sims, cap, 1.0, 6, m * sims, 0)
        kids, cnt, _ = orc.batch_mcts(lg, one, 1, wb, p, 900 + g)
        vs = [kids[j].visits for j in range(cnt[0])]
        sub = (TaflPlay * 1)()
        if vs and max(vs) > 0 and one[0].status == 0:
            C.memmove(C.byref(sub[0]), C.byref(kids[vs.index(max(vs))].play), C.sizeof(TaflPlay))
        assert pu.play_tuple4(sub[0]) == want[m][g], (name, m)
        orc.batch_step(lg, one, 1, wb, sub)
    assert bytes(one[0]) == bytes(fb[g])


def test_full_size_13x13_properties_65536():
    """BASELINE configs[4] at full size: 65 536 concurrent 13x13 games in the dense 13-column search layout - conservation properties,
    shard invariance and oracle spot ids, as for the 11x11 headline."""
    rules, fen, wb, n, lg = _mk("copenhagen13")
    G, sims, cap, seed = 65536, 6, 96, 3
    glg = gpu_logic(rules, n, wb)
    big = glg.new_batch(G, fen)
    big.mcts_run(sims, 1.0, seed, cap, game_id_base=0)
    kids, cnt = big.mcts_root_children(16)
    st = big.mcts_stats()
    assert st.sims == G * sims and st.faults == 0
    assert st.rollouts + st.terminal_hits == st.sims and sum(st.reason_hist) == st.rollouts
    for g in range(0, G, 97):
        assert sum(kids[g * 16 + j].visits for j in range(cnt[g])) == sims - 1
    quarter = glg.new_batch(G // 4, fen)
    quarter.mcts_run(sims, 1.0, seed, cap, game_id_base=3 * (G // 4))
    qk, qc = quarter.mcts_root_children(16)
    for g in range(0, G // 4, 53):
        assert _kids(qk, qc, g, 16) == _kids(kids, cnt, 3 * (G // 4) + g, 16), g
    p = TaflMctsParams(sims, cap, 1.0, seed, 0, 0)
    one = pu.start_states(orc, fen, rules.starting_side, wb, 1)
    for gid in (0, 65, 32767, 65535):
        assert _kids(kids, cnt, gid, 16) == _oracle_kids(lg, one[0], wb, p, gid), gid
    res = big.rollout(7, 0, 200, 0)
    oneres = orc.batch_rollout(lg, one, 1, wb, 7, 0, 200, 4097)
    assert (oneres[0].value, oneres[0].reason, oneres[0].plies) == (res[4097].value, res[4097].reason, res[4097].plies)


def test_training_tensor_writers():
    """board_to_matrix (game/main.rs:55-83) and the policy targets of src/mcts.py:40-53 written on the device,
    to host buffers and straight into torch tensors (device pointers)."""
    import torch
    rng = random.Random(17)
    for name in ("copenhagen11", "brandubh7", "copenhagen13", "tablut9"):
        rules, fen, wb, n, lg = _mk(name)
        G = 300
        states = pu.random_board_states(rng, n, wb, G)
        b = gpu_batch(rules, n, wb, states, G)
        enc = b.encode_boards()
        t = torch.zeros((G, n, n), dtype=torch.uint8, device="cuda")
        b.encode_boards(out_device_ptr=t.data_ptr())
        tl = t.cpu().flatten().tolist()
        assert tl == list(enc), name
        for g in range(0, G, 11):
            want = orc.GameState.from_abi(states[g], wb).board_to_matrix()
            got = [list(enc[g * n * n + r * n:g * n * n + (r + 1) * n]) for r in range(n)]
            assert got == want, (name, g)
    # policy targets
    rules, fen, wb, n, lg = _mk("copenhagen11")
    G = 128
    b = gpu_logic(rules, n, wb).new_batch(G, fen)
    b.mcts_run(32, 1.0, 5, 128, game_id_base=3)
    host = b.mcts_policy(1.0)
    dev = b.mcts_policy_device(1.0)
    assert bytes(host) == bytes(dev)
    A = b.logic.action_size
    t = torch.zeros((G, A), dtype=torch.float64, device="cuda")
    b.mcts_policy_device(1.0, out_device_ptr=t.data_ptr())
    assert t.cpu().flatten().tolist() == list(host)
    assert bytes(b.mcts_policy(0.0)) == bytes(b.mcts_policy_device(0.0))
    # best play = first maximum of the root visit counts
    bp, bv = b.mcts_best_play()
    kids, cnt = b.mcts_root_children(256)
    for g in range(G):
        vs = [kids[g * 256 + j].visits for j in range(cnt[g])]
        assert bv[g] == max(vs) and pu.play_tuple4(bp[g]) == pu.play_tuple4(kids[g * 256 + vs.index(max(vs))].play)


@pytest.mark.parametrize("name,G,sims", [("copenhagen11", 200, 70), ("brandubh7", 130, 150), ("copenhagen13", 70, 40)])
def test_mcts_pipelines_agree(name, G, sims):
    """The tuning fields of tafl_mcts_params.flags choose HOW a search runs, never its results: the default two-kernel pipeline
    (k_mcts_tree + k_mcts_rollout over the dense work list) with 1 .. 8 playout slots per game and the fused kernel
    (k_mcts_fused, 1 or 2 slots) run the same per-game functions: identical root statistics and counters."""
    rules, fen, wb, n, lg = _mk(name)
    states = pu.start_states(orc, fen, rules.starting_side, wb, G)
    plies = (C.c_uint32 * G)(*[(i * 3) % 50 for i in range(G)])
    orc.batch_random_advance(lg, states, G, wb, 19, plies, 5)
    results = []
    tunes = [abi.mcts_tune(0, 0), abi.mcts_tune(abi.MCTS_PIPELINE_TWO_KERNEL, 1), abi.mcts_tune(abi.MCTS_PIPELINE_TWO_KERNEL, 2),
             abi.mcts_tune(abi.MCTS_PIPELINE_TWO_KERNEL, 5), abi.mcts_tune(abi.MCTS_PIPELINE_TWO_KERNEL, 8),
             abi.mcts_tune(abi.MCTS_PIPELINE_TWO_KERNEL, 4, 3), abi.mcts_tune(abi.MCTS_PIPELINE_TWO_KERNEL, 0, 1)]
    if wb == 64:                      # the fused kernel exists for 64-bit boards only
        tunes += [abi.mcts_tune(abi.MCTS_PIPELINE_FUSED, 2), abi.mcts_tune(abi.MCTS_PIPELINE_FUSED, 1)]
    for flags in tunes:
        b = gpu_batch(rules, n, wb, states, G)
        b.mcts_run(sims, 1.0, 3, 300, game_id_base=5, flags=flags)
        kids, cnt = b.mcts_root_children(256)
        st = b.mcts_stats()
        results.append(([(kids[g * 256 + j].action, kids[g * 256 + j].visits, float(kids[g * 256 + j].q).hex()) for g in range(G) for j in range(cnt[g])],
                        list(cnt), (st.sims, st.rollouts, st.rollout_plies, st.tree_depth_sum, st.children_scanned, st.terminal_hits, st.faults),
                        list(st.reason_hist)))
        if flags == abi.mcts_tune(abi.MCTS_PIPELINE_TWO_KERNEL, 1):
            assert st.spec_issued == 0 and st.spec_hits == 0
        b.close()
    for r in results[1:]:
        assert r == results[0]
    with pytest.raises(Exception):                     # fused: at most 2 slots, 64-bit boards only
        gpu_batch(rules, n, wb, states, G).mcts_run(sims, 1.0, 3, 300, flags=abi.mcts_tune(abi.MCTS_PIPELINE_FUSED, 4 if wb == 64 else 2))
    with pytest.raises(Exception):
        gpu_batch(rules, n, wb, states, G).mcts_run(sims, 1.0, 3, 300, flags=1 << 20)


def test_batched_game_history_and_undo():
    """BatchedGame (game/game/mod.rs:75-116 for n games): random legal and illegal plays, undo, against the oracle's Game."""
    from alphazeroforhnefatafl_amd import BatchedGame
    rng = random.Random(9)
    rules, fen, wb = pu.CONFIGS["brandubh7"]
    G = 24
    bg = BatchedGame(rules, fen, G)
    og = [orc.Game(rules, fen, wb) for _ in range(G)]
    olg = orc.GameLogic(rules, 7)
    for step in range(30):
        plays = (abi.TaflPlay * G)()
        for g in range(G):
            legal = olg.all_plays(og[g].state)
            if legal and rng.random() < 0.8:
                p = rng.choice(legal)
            else:
                p = pu.random_plays(rng, 7, 1)[0]
            C.memmove(C.byref(plays[g]), C.byref(p), C.sizeof(abi.TaflPlay))
        codes, _ = bg.do_play(plays)
        for g in range(G):
            code, _st = og[g].do_play(plays[g])
            assert code == codes[g], (step, g)
        if step % 4 == 3:
            who = [g for g in range(G) if rng.random() < 0.5]
            bg.undo_last_play(who)
            for g in who:
                og[g].undo_last_play()
        cur = bg.state
        for g in range(G):
            assert bytes(cur[g]) == bytes(og[g].state.to_abi()), (step, g)
            assert len(bg.play_history[g]) == len(og[g].play_history)


@pytest.mark.parametrize("name,G", [("brandubh7", 96), ("copenhagen13", 48)])
def test_mcts_play_best_is_best_play_plus_do_play(name, G):
    """tafl_mcts_play_best (device-side self-play step) == tafl_mcts_best_play + tafl_step, and a short self-play loop stays
    in step with the oracle driven by the same plays.  (13x13: the search runs in the dense 13-column layout, the play is applied to
    the batch state in the reference's 15-column layout.)"""
    rules, fen, wb, n, lg = _mk(name)
    states = pu.start_states(orc, fen, rules.starting_side, wb, G)
    a = gpu_batch(rules, n, wb, states, G)
    ostates = pu.clone_states(states, G)
    for move in range(12):
        a.mcts_run(24, 1.0, 100 + move, 64, game_id_base=3)
        want_plays, want_visits = a.mcts_best_play()
        plays, eff = a.mcts_play_best()
        live = [g for g in range(G) if want_visits[g] > 0]
        for g in range(G):
            if want_visits[g] > 0:
                assert pu.play_tuple4(plays[g]) == pu.play_tuple4(want_plays[g]) and eff[g].code == 0
            else:
                assert eff[g].code != 0
        sub = (abi.TaflPlay * G)()
        for g in live:
            C.memmove(C.byref(sub[g]), C.byref(want_plays[g]), C.sizeof(abi.TaflPlay))
        oeff = orc.batch_step(lg, ostates, G, wb, sub)
        cur = a.download()
        for g in range(G):
            if g in live:
                assert pu.effects_tuple(oeff[g]) == pu.effects_tuple(eff[g]), (move, g)
        # games without a play were not touched by the device; undo the oracle's rejected empty play bookkeeping (none: rejected plays change nothing)
        assert pu.states_equal(cur, ostates, G), pu.first_state_diff(cur, ostates, G)


@pytest.mark.parametrize("name,G,sims", [("copenhagen11", 96, 150), ("brandubh7", 128, 120), ("copenhagen13", 40, 60)])
def test_mcts_first_play_urgency_flag_vs_oracle(name, G, sims):
    """TAFL_MCTS_FLAG_FPU_INF (src/mcts.rs:49-51,187): unvisited actions score +inf, new nodes start with visits 1.  The sketch cannot
    run, so the mode is pinned by the oracle's twin only ("parity unpinned" against the reference); GPU == oracle bit for bit."""
    rules, fen, wb, n, lg = _mk(name)
    states = pu.start_states(orc, fen, rules.starting_side, wb, G)
    plies = (C.c_uint32 * G)(*[(i * 7) % 33 for i in range(G)])
    orc.batch_random_advance(lg, states, G, wb, 4, plies, 11)
    K = 24                                     # oracle on the first K games (it is slow), the GPU on all of them
    p = TaflMctsParams(sims, 256, 1.0, 6, 0, abi.MCTS_FLAG_FPU_INF)
    ok, on, _ = orc.batch_mcts(lg, states, K, wb, p, 11)
    results = []
    for tune in (0, abi.mcts_tune(abi.MCTS_PIPELINE_FUSED if wb == 64 else abi.MCTS_PIPELINE_TWO_KERNEL, 2), abi.mcts_tune(abi.MCTS_PIPELINE_TWO_KERNEL, 8, 1)):
        b = gpu_batch(rules, n, wb, states, G)
        b.mcts_run(sims, 1.0, 6, 256, game_id_base=11, flags=abi.MCTS_FLAG_FPU_INF | tune)
        gk, gn = b.mcts_root_children(256)
        st = b.mcts_stats()
        assert st.sims == G * sims and st.faults == 0
        results.append([(gk[g * 256 + j].action, gk[g * 256 + j].visits, float(gk[g * 256 + j].q).hex()) for g in range(G) for j in range(gn[g])])
        for g in range(K):
            assert on[g] == gn[g]
            for j in range(on[g]):
                x, y = ok[g * 256 + j], gk[g * 256 + j]
                assert (x.action, x.visits, float(x.q).hex()) == (y.action, y.visits, float(y.q).hex()), (name, g, j)
        b.close()
    assert results[0] == results[1] == results[2]
    # and it is a different search from the default one
    b = gpu_batch(rules, n, wb, states, G)
    b.mcts_run(sims, 1.0, 6, 256, game_id_base=11)
    gk, gn = b.mcts_root_children(256)
    assert results[0] != [(gk[g * 256 + j].action, gk[g * 256 + j].visits, float(gk[g * 256 + j].q).hex()) for g in range(G) for j in range(gn[g])]


def _tafl_fmix32(h):
    h &= 0xFFFFFFFF; h ^= h >> 16; h = (h * 0x85EBCA6B) & 0xFFFFFFFF; h ^= h >> 13; h = (h * 0xC2B2AE35) & 0xFFFFFFFF; h ^= h >> 16
    return h


def _tie_pick(seed, gid, ties):
    """taflmix32 word of (tie_seed, global game id) -> index among the maxima (include/taflhip.h: tafl_mcts_policy_device_ex)."""
    f = _tafl_fmix32
    slo, shi, glo, ghi = seed & 0xFFFFFFFF, seed >> 32, gid & 0xFFFFFFFF, gid >> 32
    h0 = f(slo ^ f(shi + 0x9E3779B9)); h1 = f(shi ^ f(slo + 0x7F4A7C15))
    lo = f(f(h0 ^ glo) + ghi); hi = f(f(h1 ^ ghi) + glo * 0x9E3779B1)
    h = f(lo ^ f(hi + 0x7A1E5EED))
    return (h * ties) >> 32


def test_policy_for_any_temperature_and_seeded_tie_break():
    """getActionProb (src/mcts.py:40-53) on the device: counts ** (1 / temp) / sum for any temp > 0 (device pow: compared with the
    host's libm within 4 ulp, exact for temp == 1 and for integer exponents), and temp == 0 with the np.random.choice among the maxima
    replaced by a seeded, sharding-independent draw (tie_seed; 0 = the first maximum)."""
    import math
    rules, fen, wb, n, lg = _mk("copenhagen11")
    G, sims, base = 96, 40, 1000
    b = gpu_logic(rules, n, wb).new_batch(G, fen)
    b.mcts_run(sims, 1.0, 5, 128, game_id_base=base)
    A = b.logic.action_size
    visits = b.mcts_root_visits()
    for temp in (1.0, 0.5, 0.25, 2.0, 0.7, 1.3):
        dev = b.mcts_policy_device(temp)
        host = b.mcts_policy(temp)                      # host: libm pow on the downloaded counts, same operation order
        exact = temp in (1.0, 0.5, 0.25)
        for g in range(G):
            cnt = visits[g * A:(g + 1) * A]
            ex = 1.0 / temp
            w = [float(c) ** ex for c in cnt]           # Python: x ** (1. / temp)
            ssum = float(sum(w))
            for a in range(A):
                d, h = dev[g * A + a], host[g * A + a]
                want = w[a] / ssum
                if exact:
                    assert d == want == h, (temp, g, a)
                else:
                    assert h == want
                    assert d == want or abs(d - want) <= 4 * math.ulp(want), (temp, g, a, d, want)
    # temp == 0: one-hot on a maximum
    first = b.mcts_policy_device(0.0)
    assert bytes(first) == bytes(b.mcts_policy(0.0))
    seeded = b.mcts_policy_device(0.0, tie_seed=77, game_id_base=base)
    moved = 0
    for g in range(G):
        cnt = visits[g * A:(g + 1) * A]
        mx = max(cnt)
        maxima = [a for a in range(A) if cnt[a] == mx]
        row = seeded[g * A:(g + 1) * A]
        assert sum(row) == 1.0 and sorted(set(row)) == [0.0, 1.0]
        want = maxima[_tie_pick(77, base + g, len(maxima))] if len(maxima) > 1 else maxima[0]
        assert row[want] == 1.0, (g, maxima, want)
        assert first[g * A + maxima[0]] == 1.0
        moved += want != maxima[0]
    assert moved > 0                                      # ties exist at 40 simulations and the seed moves some of them
    # the same draw from a shard of the batch with its own base
    half = gpu_logic(rules, n, wb).new_batch(G // 2, fen)
    half.mcts_run(sims, 1.0, 5, 128, game_id_base=base + G // 2)
    hs = half.mcts_policy_device(0.0, tie_seed=77, game_id_base=base + G // 2)
    assert list(hs) == list(seeded[(G // 2) * A:])


def test_context_refuses_to_die_before_its_batches():
    from alphazeroforhnefatafl_amd._lib import lib
    from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
    rules, fen, wb, n, lg = _mk("brandubh7")
    logic = BatchedGameLogic(rules, n, wb)
    b = logic.new_batch(10, fen)
    assert lib().tafl_ctx_destroy(logic._h) != 0          # library level: refused while a batch is alive
    counts, _ = b.iter_plays(want_masks=False)            # the batch still works
    assert counts[0] == 40
    logic.close()                                         # host mirror: closes its batches first
    assert not b._h and not logic._h
    # range checks of upload / download do not wrap
    logic2 = BatchedGameLogic(rules, n, wb)
    b2 = logic2.new_batch(4, fen)
    st = b2.download()
    assert lib().tafl_batch_upload(b2._h, st, 0xFFFFFFFF, 2) != 0
    assert lib().tafl_batch_download(b2._h, st, 3, 0xFFFFFFFE) != 0
    logic2.close()
