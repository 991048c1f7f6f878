"""Inputs that make the repetition tracker of a playout matter, and what the oracle gives for them: shared by
tests/test_hostsim_value_only.py (CPU) and tests/test_gpu_value_only.py.

The states are those of the back-and-forth sequences of tests/test_hostsim_rare.py::test_repetition_sequences, cut at every ply, each in one of
ten variants of its tracker (`VARIANTS`): as it is; `reps` one below n_repetitions for the side to move, for the other side, for both; a
set mid-pair flag of either side; a ring cut down to 0 .. 3 entries; an entry with the captured bit; a ring whose entries do not alternate
sides; an entry that is no play on the board.  A uniform-random playout repeats the play of four plies ago in about one case in a hundred,
so the batch is put together slot by slot: game g of a batch plays with the key (seed, base + g, sim), and `workload` looks, with the
ORACLE alone, for (slot, snapshot) pairs whose first ply repeats the play of four plies ago; such a slot keeps either the armed form of the
snapshot (a repetition ending) or another variant of it (a near miss: the same ply against another tracker).  The other slots hold the
variants in turn.  Nothing here looks at an engine under test."""
import collections
import ctypes as C
import functools
import random

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflPlay, TaflState
from oracle import oracle as orc
from tests import parity_util as pu
from tests import rare_workloads as rw

Config = collections.namedtuple("Config", "name rules n wb preset fen")
CONFIGS = {c.name: c for c in (
    Config("copenhagen11", abi.rules.COPENHAGEN, 11, 128, True, abi.boards.COPENHAGEN),      # preset <4, 11>; repetition loses
    Config("brandubh7", abi.rules.BRANDUBH, 7, 64, True, abi.boards.BRANDUBH),               # preset <2, 7>; repetition loses
    Config("tablut9", abi.rules.TABLUT, 9, 128, False, abi.boards.TABLUT),                   # run-time <4, 11>; repetition draws
    Config("copenhagen13", abi.rules.COPENHAGEN, 13, 256, True, abi.boards.COPENHAGEN13),    # preset, dense <6, 13> (CPU test only)
)}
G_FULL, SEED, BASE = 641, 1, 100                 # 641 = ten waves and one lane
CPU_CAP, GPU_CAP = 12, 80
# repetition endings: the asserted floor; what the slot search aims for as (endings, near misses), less on the large board whose ruleset the
# 11x11 board covers; the bound of the search
FLOOR, WANTED, ROTATIONS = 32, {None: (40, 36), "copenhagen13": (12, 9)}, 400
VARIANTS = 10
MCTS_G, MCTS_SIMS = 513, 16


def is_repetition(t):
    """t: rare_workloads.result_tuple = (value, status, reason, winner, plies); a rollout result's draw reasons are 8 + DrawReason"""
    return (t[1] == abi.WIN and t[2] == abi.WIN_REPETITION) or (t[1] == abi.DRAW and t[2] == 8 + abi.DRAW_REPETITION)


def _snapshots(cfg, games=48, plies=28):
    """Ongoing states of `games` shuffles, one per game and ply (the sequences of test_repetition_sequences, with its interruptions)."""
    lg = orc.GameLogic(cfg.rules, cfg.n)
    rng = random.Random(12)
    states = pu.start_states(orc, cfg.fen, cfg.rules.starting_side, cfg.wb, games)
    a_plays = lg.all_plays(orc.GameState(cfg.fen, abi.ATTACKER, cfg.wb))
    d_plays = lg.all_plays(orc.GameState(cfg.fen, abi.DEFENDER, cfg.wb))

    def rev(p):
        t = abi.play_to(p)
        return TaflPlay(t[0], t[1], p.axis, -p.disp)

    picks = []
    for _ in range(games):
        pa = rng.choice(a_plays)
        picks.append((pa, rng.choice([p for p in d_plays if abi.play_to(p) != abi.play_to(pa)])))
    first = abi.ATTACKER if cfg.rules.starting_side == abi.ATTACKER else abi.DEFENDER
    out = []
    for ply in range(plies):
        plays = (TaflPlay * games)()
        for g in range(games):
            pa, pd = picks[g]
            seq = [pa, pd, rev(pa), rev(pd)] if first == abi.ATTACKER else [pd, pa, rev(pd), rev(pa)]
            plays[g] = pu.random_plays(rng, cfg.n, 1)[0] if rng.random() < 0.03 else seq[ply % 4]
        orc.batch_step(lg, states, games, cfg.wb, plays)
        out += [TaflState.from_buffer_copy(bytes(states[g])) for g in range(games) if states[g].status == abi.ONGOING]
    return out


def _variant(cfg, st, k):
    """Variant k of the tracker of state `st` (a copy)."""
    s = TaflState.from_buffer_copy(bytes(st))
    below = cfg.rules.repetition_rule[0] - 1
    mover_def = s.side_to_play == abi.DEFENDER

    def arm(defender):
        if defender:
            s.defender_reps, s.defender_mid_pair = below, 0
        else:
            s.attacker_reps, s.attacker_mid_pair = below, 0

    v = k % VARIANTS
    if v in (1, 2, 4, 5, 6, 7, 8):
        arm(mover_def)                            # one counted repetition of the side to move ends the game
    if v in (3, 8):
        arm(not mover_def)
    if v == 2:                                    # mid-pair set: the next hit of the side to move does not count
        if mover_def: s.defender_mid_pair = 1
        else: s.attacker_mid_pair = 1
    if v == 3:
        if mover_def: s.attacker_mid_pair = 1
        else: s.defender_mid_pair = 1
    if v == 9:
        s.attacker_mid_pair = s.defender_mid_pair = 1
    if v == 4:                                    # a ring of 0 .. 3 entries: the oldest are None
        for i in range(4 - (k // VARIANTS) % 4):
            s.rep_ring[i] = 0
    if v == 5:                                    # the entry the first ply is compared with carries the captured bit
        i = (k // VARIANTS) % 2
        if s.rep_ring[i]:                         # (None is all zeros: a word with bits but without bit 31 is no ring entry)
            s.rep_ring[i] |= 1 << 29
    if v == 6:                                    # entries that do not alternate sides
        if (k // VARIANTS) % 2: s.rep_ring[1] = s.rep_ring[0]
        else: s.rep_ring[0], s.rep_ring[1] = s.rep_ring[1], s.rep_ring[0]
    if v == 7 and s.rep_ring[0]:                  # no play on this board: a row outside it / displacement 0 / a slide off the board
        e, j = s.rep_ring[0], (k // VARIANTS) % 3
        s.rep_ring[0] = (e & ~(0xFF << 16)) | (200 << 16) if j == 0 else (e & ~0xFF) if j == 1 else (e & ~0xFF) | 0x7F
    return s


def _batch(states):
    arr = (TaflState * len(states))()
    sz = C.sizeof(TaflState)
    for g, st in enumerate(states):
        C.memmove(C.byref(arr, g * sz), C.byref(st), sz)
    return arr


NEAR_VARIANTS = (2, 4, 5, 6, 7, 3, 9, 0, 8)


@functools.lru_cache(maxsize=None)
def workload(name, G=G_FULL):
    """(states, slots filled with a repetition ending, slots filled with a near miss).  The search offers every slot the ARMED form (variant
    1) of one snapshot after the other; where the oracle ends that playout by repetition the slot is a hit - its first ply repeats the play
    of four plies ago - and hits keep, in turn, the armed form (a repetition ending) or another variant of the same snapshot (a near miss:
    the same first ply against a mid-pair flag, a cut ring, a captured bit, ... - whatever the oracle makes of it)."""
    cfg = CONFIGS[name]
    lg = orc.GameLogic(cfg.rules, cfg.n)
    snaps = _snapshots(cfg)
    K = len(snaps)
    armed = [_variant(cfg, st, 1) for st in snaps]
    wanted, near = WANTED.get(name, WANTED[None])
    first = [(g * 7) % K for g in range(G)]
    fixed, n_end, n_near = {}, 0, 0
    for r in range(ROTATIONS):
        picks = [(first[g] + r * 13) % K for g in range(G)]
        res = orc.batch_rollout(lg, _batch([armed[k] for k in picks]), G, cfg.wb, SEED, rw.ROLLOUT_SIM, CPU_CAP, BASE)
        for g in range(G):
            if g in fixed or not is_repetition(rw.result_tuple(res[g])):
                continue
            if n_end <= n_near or n_near >= near:
                fixed[g], n_end = armed[picks[g]], n_end + 1
            else:
                fixed[g] = _variant(cfg, snaps[picks[g]], NEAR_VARIANTS[n_near % 9] + VARIANTS * (n_near // 9))
                n_near += 1
        if n_end >= wanted and n_near >= near:
            break
    return _batch([fixed[g] if g in fixed else _variant(cfg, snaps[first[g]], g) for g in range(G)]), n_end, n_near


@functools.lru_cache(maxsize=None)
def expectations(name, cap):
    """{batch size: (states, G, {SEED: [result tuple]})} for 641, 65 and 1 games (prefixes of one list: game g keeps its key)."""
    cfg = CONFIGS[name]
    lg = orc.GameLogic(cfg.rules, cfg.n)
    states = workload(name)[0]
    out = {}
    for count in (G_FULL, 65, 1):
        sub = pu.clone_states(states, count)
        out[count] = (sub, count, rw._oracle_rollouts(cfg, lg, sub, count, (SEED,), cap, BASE))
    return out


def repetition_endings(name, cap):
    return sum(is_repetition(t) for t in expectations(name, cap)[G_FULL][2][SEED])


def advance_plies(G):
    return (C.c_uint32 * G)(*[g % 7 + 1 for g in range(G)])


@functools.lru_cache(maxsize=None)
def advance_expectation(name):
    cfg = CONFIGS[name]
    states = workload(name)[0]
    want = pu.clone_states(states, G_FULL)
    orc.batch_random_advance(orc.GameLogic(cfg.rules, cfg.n), want, G_FULL, cfg.wb, rw.ADVANCE_SEED, advance_plies(G_FULL), rw.ADVANCE_BASE)
    return want


def mcts_params(flags=0):
    return abi.TaflMctsParams(MCTS_SIMS, GPU_CAP, rw.MCTS_CPUCT, rw.MCTS_SEED, 0, flags)


@functools.lru_cache(maxsize=None)
def mcts_expectation(name):
    cfg = CONFIGS[name]
    states = workload(name)[0]
    sub = pu.clone_states(states, MCTS_G)
    return sub, rw.oracle_mcts(orc.GameLogic(cfg.rules, cfg.n), sub, MCTS_G, cfg.wb, mcts_params(), rw.MCTS_BASE)
