"""Rare-rule workloads for the playout kernels, the oracle's expectations for them and ONE comparison code for two engines.

The playout engine (csrc/tafl_fast.hpp) runs in two forms: with run-time `Consts` (any ruleset) and as the preset instantiations
(Copenhagen 11x11, Brandubh 7x7, Copenhagen 13x13 in the dense 6-limb layout) in which every mask and bit index is a literal and the
rule branches are folded away.  Host-sim (tests/hostsim) compiles the run-time form only, so the preset instantiations can be checked
on the device alone.  This module builds crafted positions from which playouts end in the rare outcomes within a few plies (enclosure,
exit fort, shieldwall captures, no plays, all captured), asks the oracle what must come out, and compares an *engine adapter* against
it: `HostSimEngine` (CPU; proves the workloads and this code) and `GpuEngine` (the library through the C-ABI).  Every comparison is
bit-exact; the coverage conditions are evaluated on the oracle's results only.  The module itself uses no GPU.

Checks (tests/test_hostsim_rare_workloads.py, tests/test_gpu_rare_rollouts.py):
  a. rollouts from the crafted list: (value, status, reason, winner, plies) per game, batch unchanged; list lengths 1 mod 64, 65, 1
  b. in-place playouts (random_advance) of 1 .. 7 plies: states byte for byte (capture sets, T-layout upkeep, repetition ring)
  c. three-ply playouts from shieldwall positions under 12 seeds (the window pre-filter of the fast engine)
  d. MCTS from a crafted mix: every game's root children and all counters (k_mcts_rollout, the terminal handling of the tree step)
The code that makes a move and goes on, from the crafted mix of (d), in which the oracle's own runs end games by enclosure, exit fort, no
plays and all captured within 3 - 4 moves (tests/test_hostsim_rare_workloads.py, tests/test_gpu_rare_runs.py):
  e. the self-play run (Ops::selfplay_advance_impl, on 13x13 between two restrides): plays [move][game], final states, sims, no fault; both
     pipelines of the device; the first game a rare rule ended, alone under its global id
  f. the recording run and finalize: lens, every example field, z and final, the counters, with temp_moves 0 and n_moves and in two pieces;
     on the device the gather of the ended games' examples under all eight symmetries
  g. one guided search per game (Guided::step's term): root children as (action, visits, Q bits), sims, predicts, terminal hits; on the
     device the dense getters
  h. guided self-play at each game's own pace (Guided::selfplay_step): plays, moves, states, examples against gselfplay_util.oracle_run
  i. device only (host-sim has no advance entry point): mcts_advance / gmcts_advance onto the first-maximum child - terminal by a rare rule
     for a quarter of the games, a shieldwall capture of four pieces among them - against the oracle's step, then a keep-search
"""
import collections
import ctypes as C
import functools
import random
from concurrent.futures import ThreadPoolExecutor

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflMctsParams, TaflMctsStats, TaflPlay, TaflRootChild, TaflState
from oracle import oracle as orc
from tests import examples_util as xu
from tests import gselfplay_util as gsu
from tests import guided_util as gu
from tests import parity_util as pu
from tests.stub_net import matrix_bytes_of

Config = collections.namedtuple("Config", "name rules n wb preset")

CONFIGS = {c.name: c for c in (
    # the three preset instantiations (what the benchmark runs)
    Config("copenhagen11", abi.rules.COPENHAGEN, 11, 128, True),         # preset 4 limbs x 11 columns
    Config("copenhagen13", abi.rules.COPENHAGEN, 13, 256, True),         # preset, dense 6 x 13; the batch stays in 8 x 15
    Config("brandubh7", abi.rules.BRANDUBH, 7, 64, True),                # preset 2 x 7: fused and two-kernel searches
    # their run-time twins: a failure of a preset alone is a folding error, a failure of both is the engine's
    Config("copenhagen11_u256", abi.rules.COPENHAGEN, 11, 256, False),   # run-time <8, 15>
    Config("tablut9", abi.rules.TABLUT, 9, 128, False),                  # run-time 4 x 11
    Config("koch7_u128", abi.rules.KOCH, 7, 128, False),                 # run-time 4 x 11 on a 7-board
)}
PRESETS = tuple(c.name for c in CONFIGS.values() if c.preset)
TWINS = tuple(c.name for c in CONFIGS.values() if not c.preset)

# positions that once told an engine from the oracle, pinned as explicit states: {config name: [(att limbs, deff limbs, side to play)]}
PINNED = {}

ROLLOUT_SEEDS, ROLLOUT_SIM, ROLLOUT_CAP, ROLLOUT_BASE = (1, 2), 3, 80, 100
ADVANCE_SEED, ADVANCE_BASE = 5, 11
HINT_SEEDS, HINT_CAP, HINT_COUNT = tuple(range(100, 112)), 3, 150
MCTS_CAP, MCTS_CPUCT, MCTS_SEED, MCTS_BASE, MCTS_WIDTH = 80, 1.0, 2, 7, 256
STAT_FIELDS = ("sims", "rollouts", "rollout_plies", "tree_depth_sum", "children_scanned", "terminal_hits", "faults")

# Floors of check (a) on the oracle's (status == WIN) reasons, summed over both seeds of the full list.  The oracle gives, with
# Random(41) and 128 positions per kind (test_hostsim_rare_workloads.py asserts that every floor is at least half of what it gives):
#   copenhagen11 (641 games): ENCLOSED 14, EXIT_FORT 31, WIN_NO_PLAYS 16, ALL_CAPTURED 21   (KING_ESCAPED 302, KING_CAPTURED 8)
#   copenhagen13 (641 games): ENCLOSED 19, EXIT_FORT 38, WIN_NO_PLAYS 10, ALL_CAPTURED 14   (KING_ESCAPED 223, KING_CAPTURED 6)
#   brandubh7 (513 games):    ENCLOSED 39, WIN_NO_PLAYS 20, ALL_CAPTURED 66, KING_CAPTURED 124 (KING_ESCAPED 464, WIN_REPETITION 1)
# Each floor is the larger of: 8 / 15 / 5 / 5 (Copenhagen) and 15 / 8 / 20 / 30 (Brandubh), and half of the figure above rounded up.
ROLLOUT_FLOORS = {
    "copenhagen11": {abi.ENCLOSED: 8, abi.EXIT_FORT: 16, abi.WIN_NO_PLAYS: 8, abi.ALL_CAPTURED: 11},
    "copenhagen13": {abi.ENCLOSED: 10, abi.EXIT_FORT: 19, abi.WIN_NO_PLAYS: 5, abi.ALL_CAPTURED: 7},
    "brandubh7": {abi.ENCLOSED: 20, abi.WIN_NO_PLAYS: 10, abi.ALL_CAPTURED: 33, abi.KING_CAPTURED: 62},
}
# Floors of check (d) on the oracle's counters.  The oracle gives, with Random(43): terminal_hits 1 133 / 458 / 1 368 on 11x11 / 13x13 /
# Brandubh; reason_hist of 11x11: 34 exit forts, 19 all captured, 9 enclosed, 2 no plays; of 13x13: 12 exit forts, 10 all captured,
# 3 enclosed; of Brandubh: 146 all captured, 9 enclosed, 3 no plays; roots left out: 0 of 96, 0 of 64, 1 of 72.
MCTS_FLOORS = {
    "copenhagen11": {"terminal_hits": 100, abi.ENCLOSED: 3, abi.EXIT_FORT: 8},
    "copenhagen13": {"terminal_hits": 100, abi.ENCLOSED: 3, abi.EXIT_FORT: 8},
    "brandubh7": {"terminal_hits": 100, abi.ENCLOSED: 3},
}
RUN_SSEED, RUN_K = 11, 64                         # checks (e) .. (i): sample seed of the draws, max_children of the examples
G_CPUCT, G_EDGES, H_TEMP = 1.25, 256, 2           # guided: c_puct, edges_per_node; temp_moves of the guided self-play run
RARE_REASONS = (abi.ENCLOSED, abi.EXIT_FORT, abi.ALL_CAPTURED, abi.WIN_NO_PLAYS)
Recording = collections.namedtuple("Recording", "plays states lens example counters sims faults gather close")
# Floors of checks (e) and (f): games that the oracle's run itself ended, by win reason, and "later": games that made two moves or more and
# then ended.  Every floor is half of what the oracle gives, rounded up (a re-measurement replaces the figure and the floor with it, by the
# same rule).  The oracle loop (examples_util.oracle_record, S = 48 / 32 on 13x13, 4 / 3 moves, cap 80, seed 2, base 7) gives, temp_moves 0:
#   copenhagen11 (96 games): 34 ended, 27 after one move: ENCLOSED 10, ALL_CAPTURED 7, EXIT_FORT 7, NO_PLAYS 4, KING_CAPTURED 3, KING_ESCAPED 3; later 7
#   copenhagen13 (64):       19 ended, 16 after one:      EXIT_FORT 7, ENCLOSED 4, ALL_CAPTURED 4, KING_ESCAPED 2, KING_CAPTURED 1, NO_PLAYS 1; later 3
#   brandubh7 (71 of 72):    41 ended, 31 after one:      KING_CAPTURED 12, ALL_CAPTURED 10, ENCLOSED 8, NO_PLAYS 7, KING_ESCAPED 4; later 10
#   (twins: copenhagen11_u256 as copenhagen11; tablut9: ALL_CAPTURED 13, KING_ESCAPED 10, KING_CAPTURED 7, later 12; koch7_u128: KING_CAPTURED 11,
#   ENCLOSED 9, ALL_CAPTURED 9, NO_PLAYS 7, KING_ESCAPED 3, later 8); widest root 47 / 31 / 44 visited children: nothing overflows K = 64.
RUN_FLOORS = {
    "copenhagen11": {abi.ENCLOSED: 5, abi.EXIT_FORT: 4, abi.ALL_CAPTURED: 4, abi.WIN_NO_PLAYS: 2, "later": 4},
    "copenhagen13": {abi.ENCLOSED: 2, abi.EXIT_FORT: 4, abi.ALL_CAPTURED: 2, abi.WIN_NO_PLAYS: 1, "later": 2},
    "brandubh7": {abi.ENCLOSED: 4, abi.ALL_CAPTURED: 5, abi.WIN_NO_PLAYS: 4, "later": 5},
    # the run-time twins, by the same rule (Tablut has no enclosure, exit fort or no-plays win: its floors hold the endings it has)
    "copenhagen11_u256": {abi.ENCLOSED: 5, abi.EXIT_FORT: 4, abi.ALL_CAPTURED: 4, abi.WIN_NO_PLAYS: 2, "later": 4},
    "tablut9": {abi.ALL_CAPTURED: 7, abi.KING_ESCAPED: 5, abi.KING_CAPTURED: 4, "later": 6},
    "koch7_u128": {abi.ENCLOSED: 5, abi.ALL_CAPTURED: 5, abi.WIN_NO_PLAYS: 4, "later": 4},
}
# ... and with temp_moves = n_moves, sample seed 11 (non-argmax picks 155 of 305, 90 of 162, 75 of 196 game-moves):
#   copenhagen11: 29 ended, 24 after one: ENCLOSED 10, EXIT_FORT 8, ALL_CAPTURED 7, KING_ESCAPED 2, NO_PLAYS 1, KING_CAPTURED 1; later 5
#   copenhagen13: 17 ended, 14 after one: EXIT_FORT 6, ENCLOSED 4, ALL_CAPTURED 3, KING_ESCAPED 2, KING_CAPTURED 1, NO_PLAYS 1; later 3
#   brandubh7:    35 ended, 25 after one: KING_CAPTURED 12, ENCLOSED 8, ALL_CAPTURED 7, NO_PLAYS 6, KING_ESCAPED 2; later 10
RUN_FLOORS_SAMPLED = {
    "copenhagen11": {abi.ENCLOSED: 5, abi.EXIT_FORT: 4, abi.ALL_CAPTURED: 4, abi.WIN_NO_PLAYS: 1, "later": 3},
    "copenhagen13": {abi.ENCLOSED: 2, abi.EXIT_FORT: 3, abi.ALL_CAPTURED: 2, abi.WIN_NO_PLAYS: 1, "later": 2},
    "brandubh7": {abi.ENCLOSED: 4, abi.ALL_CAPTURED: 4, abi.WIN_NO_PLAYS: 3, "later": 5},
    # twins: copenhagen11_u256 as copenhagen11; tablut9 KING_ESCAPED 10, ALL_CAPTURED 8, KING_CAPTURED 7, later 9; koch7_u128 ENCLOSED 8,
    # KING_CAPTURED 8, ALL_CAPTURED 6, NO_PLAYS 6, KING_ESCAPED 4, later 8
    "copenhagen11_u256": {abi.ENCLOSED: 5, abi.EXIT_FORT: 4, abi.ALL_CAPTURED: 4, abi.WIN_NO_PLAYS: 1, "later": 3},
    "tablut9": {abi.ALL_CAPTURED: 4, abi.KING_ESCAPED: 5, abi.KING_CAPTURED: 4, "later": 5},
    "koch7_u128": {abi.ENCLOSED: 4, abi.ALL_CAPTURED: 3, abi.WIN_NO_PLAYS: 3, "later": 4},
}
# Floor of check (g) on the terminal hits that GameLogic.gmcts itself counts (S = 32 / 24 on 13x13, c_puct 1.25, salts (3 g + 1) % 256): the
# oracle gives (sims, predicts, terminal hits) = (3 072, 2 505, 567) on 11x11, (1 536, 1 230, 306) on 13x13, (2 272, 1 675, 597) on Brandubh
# (tablut9 392, koch7_u128 595 terminal hits); half of it, rounded up.
GUIDED_HIT_FLOORS = {"copenhagen11": 284, "copenhagen13": 153, "brandubh7": 299, "copenhagen11_u256": 284, "tablut9": 196, "koch7_u128": 298}
# Floors of check (h) on gselfplay_util.oracle_run (3 moves, 4 on 7x7, temp_moves 2, sample seed 11, base 7), half of:
#   copenhagen11: ENCLOSED 8, EXIT_FORT 7, KING_ESCAPED 4, NO_PLAYS 2, KING_CAPTURED 1, ALL_CAPTURED 1; 17 games ended by their first move, later 6
#   copenhagen13: EXIT_FORT 7, ALL_CAPTURED 4, ENCLOSED 3, NO_PLAYS 1, KING_ESCAPED 1; 13 by their first move, later 3
#   brandubh7:    ENCLOSED 9, KING_ESCAPED 6, ALL_CAPTURED 6, NO_PLAYS 4, KING_CAPTURED 1; 18 by their first move, later 8
GSELFPLAY_FLOORS = {
    "copenhagen11": {abi.ENCLOSED: 4, abi.EXIT_FORT: 4, "later": 3},
    "copenhagen13": {abi.ENCLOSED: 2, abi.EXIT_FORT: 4, "later": 2},
    "brandubh7": {abi.ENCLOSED: 5, "later": 4},
    # twins: copenhagen11_u256 as copenhagen11; tablut9 KING_ESCAPED 15, ALL_CAPTURED 4, KING_CAPTURED 1, later 13; koch7_u128 as brandubh7
    "copenhagen11_u256": {abi.ENCLOSED: 4, abi.EXIT_FORT: 4, "later": 3},
    "tablut9": {abi.KING_ESCAPED: 8, abi.ALL_CAPTURED: 2, "later": 7},
    "koch7_u128": {abi.ENCLOSED: 5, "later": 4},
}
# Floors of check (i) on the oracle's step of the first-maximum root child: (children that are terminal by enclosure, exit fort, all captured
# or no plays; plays that capture two pieces or more), half of what the oracle gives, after check (d)'s search / after check (g)'s:
#   copenhagen11: 25 (ENCLOSED 10, ALL_CAPTURED 6, EXIT_FORT 6, NO_PLAYS 3), 2 multi-captures (one of 4 pieces) / 19 (8, 1, 8, 2), 0
#   copenhagen13: 15 (EXIT_FORT 6, ENCLOSED 4, ALL_CAPTURED 4, NO_PLAYS 1), 0 / 15 (6, 4, 4, 1), 1
#   brandubh7:    22 (ENCLOSED 8, ALL_CAPTURED 7, NO_PLAYS 7), 0 / 15 (8, 4, 3), 0
ADVANCE_FLOORS = {
    "copenhagen11": {"mcts": (13, 1), "guided": (10, 0)},
    "copenhagen13": {"mcts": (8, 0), "guided": (8, 1)},
    "brandubh7": {"mcts": (11, 0), "guided": (8, 0)},
    # twins: copenhagen11_u256 as copenhagen11; tablut9 8 (ALL_CAPTURED), 1 / 2 (ALL_CAPTURED), 0; koch7_u128 23 (ENCLOSED 9, ALL_CAPTURED 7,
    # NO_PLAYS 7), 0 / 15 (8, 4, 3), 0
    "copenhagen11_u256": {"mcts": (13, 1), "guided": (10, 0)},
    "tablut9": {"mcts": (4, 1), "guided": (1, 0)},
    "koch7_u128": {"mcts": (12, 0), "guided": (8, 0)},
}
MCTS_MAX_LEFT_OUT = 0.05          # roots without a legal play (the search is not defined there): at most this share of the list


# ---- workloads ------------------------------------------------------------------------------------------------------------------------

def _pinned_states(cfg):
    out = []
    for att, deff, side in PINNED.get(cfg.name, ()):
        st = TaflState()
        for i, (a, d) in enumerate(zip(att, deff)):
            st.att[i], st.deff[i] = a, d
        st.side_to_play, st.side_len, st.status = side, cfg.n, abi.ONGOING
        out.append(st)
    return out


def _crafted(rng, cfg, per_kind, with_random):
    """[(kind, [TaflState])] in a fixed order of the generators (the lists depend on it)."""
    kinds = [("enclosure", pu.enclosure_positions(rng, cfg.n, cfg.wb, per_kind)),
             ("shieldwall", pu.shieldwall_positions(rng, cfg.n, cfg.wb, per_kind)),
             ("sparse", pu.sparse_endgame_positions(rng, cfg.n, cfg.wb, per_kind))]
    if cfg.n >= 9:
        kinds.append(("exit_fort", pu.exit_fort_positions(rng, cfg.n, cfg.wb, per_kind)))
    if with_random:
        arr = pu.random_board_states(rng, cfg.n, cfg.wb, per_kind)
        kinds.append(("random", [arr[i] for i in range(per_kind)]))
    return kinds


Workload = collections.namedtuple("Workload", "states G kinds")     # kinds: [(kind, first, end)]


def _workload(kinds):
    lst, spans = [], []
    for kind, states in kinds:
        spans.append((kind, len(lst), len(lst) + len(states)))
        lst += states
    return Workload(pu.states_array(lst), len(lst), spans)


def kind_of(w, g):
    return next((k for k, a, b in w.kinds if a <= g < b), "?")


@functools.lru_cache(maxsize=None)
def rollout_workload(name, per_kind=128):
    """The crafted list of checks (a) and (b): `per_kind` positions of every kind, the pinned states, and as many more synthetic boards
    as make the length 1 mod 64 (TAFL_BLOCK is 64: a last wave with a single live lane)."""
    cfg = CONFIGS[name]
    rng = random.Random(41)
    kinds = _crafted(rng, cfg, per_kind, True)
    pinned = _pinned_states(cfg)
    if pinned:
        kinds.append(("pinned", pinned))
    pad = (1 - sum(len(s) for _, s in kinds)) % 64
    if pad:
        arr = pu.random_board_states(rng, cfg.n, cfg.wb, pad)
        kinds.append(("random", [arr[i] for i in range(pad)]))
    w = _workload(kinds)
    assert w.G % 64 == 1
    return w


def sub_batch(w, count):
    """`count` games spread evenly over the list (every kind is in the 65-game batch; the lone game is the first enclosure position)."""
    idx = [0] if count == 1 else [(i * (w.G - 1)) // (count - 1) for i in range(count)]
    return pu.states_array([w.states[i] for i in idx]), idx


def advance_plies(G):
    return (C.c_uint32 * G)(*[g % 7 + 1 for g in range(G)])


@functools.lru_cache(maxsize=None)
def hint_workload(n, wb):
    """Check (c): 150 wall-ready positions; the oracle must find at least 20 legal plays that capture two or more pieces."""
    lst = pu.shieldwall_positions(random.Random(77), n, wb, HINT_COUNT)
    states = pu.states_array(lst)
    lg = orc.GameLogic(abi.rules.COPENHAGEN, n)
    oc, _ = orc.batch_movegen(lg, states, len(lst), wb)
    arr, ranks, total, _ = pu.expand_all(states, len(lst), oc)
    _, oe = orc.batch_step_kth(lg, pu.clone_states(arr, total), total, wb, ranks)
    multi = sum(1 for i in range(total) if oe[i].n_captures >= 2)
    return Workload(states, len(lst), [("shieldwall", 0, len(lst))]), multi


def hint_rules():
    """The Copenhagen preset and a ruleset next to it (walls of every piece type, no corner closing): a run-time kernel."""
    return (("preset", abi.rules.COPENHAGEN), ("runtime", abi.rules.COPENHAGEN.replace(shieldwall=(False, abi.ps_all()))))


def mcts_sims(name):
    return 32 if CONFIGS[name].n == 13 else 48


@functools.lru_cache(maxsize=None)
def mcts_workload(name):
    """Check (d): 24 positions per kind (16 on 13x13) without the synthetic boards, the pinned states, less the roots whose side to move
    has no legal play while the game is ONGOING (the oracle books n_sims - 1 faults there).  Returns (workload, left out, list size)."""
    cfg = CONFIGS[name]
    kinds = _crafted(random.Random(43), cfg, 16 if cfg.n == 13 else 24, False)
    pinned = _pinned_states(cfg)
    if pinned:
        kinds.append(("pinned", pinned))
    full = _workload(kinds)
    counts, _ = orc.batch_movegen(orc.GameLogic(cfg.rules, cfg.n), full.states, full.G, cfg.wb, want_masks=False)
    kept = [(k, [full.states[g] for g in range(a, b) if counts[g] > 0]) for k, a, b in full.kinds]
    w = _workload(kept)
    return w, full.G - w.G, full.G


# ---- the oracle's expectations (computed once per process, never modified) --------------------------------------------------------------

def result_tuple(r):
    return (r.value, r.status, r.reason, r.winner, r.plies)


def _slices(states, G, workers):
    """[(first game, its TaflState array)] of at most `workers` slices of the batch, for oracle calls side by side on host threads (ctypes
    releases the GIL in the C call).  Game g keeps the id base + g when a slice is run with base + its first game."""
    sz, per = C.sizeof(TaflState), max(1, -(-G // workers))
    raw = bytes(states)
    return [(g0, (TaflState * min(per, G - g0)).from_buffer_copy(raw[g0 * sz:(g0 + min(per, G - g0)) * sz])) for g0 in range(0, G, per)]


def _oracle_rollouts(cfg, lg, states, G, seeds, cap, base, workers=16):
    jobs = [(seed, g0, sub) for seed in seeds for g0, sub in _slices(states, G, workers)]

    def one(job):
        seed, g0, sub = job
        return [result_tuple(r) for r in orc.batch_rollout(lg, sub, len(sub), cfg.wb, seed, ROLLOUT_SIM, cap, base + g0)]

    with ThreadPoolExecutor(max_workers=workers) as ex:
        parts = list(ex.map(one, jobs))
    out = {seed: [] for seed in seeds}
    for (seed, _, _), tuples in zip(jobs, parts):
        out[seed] += tuples
    return out


def win_reason_hist(per_seed):
    """Counter of the reasons of the won games over all seeds."""
    return collections.Counter(t[2] for tuples in per_seed.values() for t in tuples if t[1] == abi.WIN)


@functools.lru_cache(maxsize=None)
def rollout_expectations(name):
    """{batch size: (states, G, {seed: [result tuple]})} for the full list, 65 games and 1 game, and the full list's win-reason histogram."""
    cfg = CONFIGS[name]
    lg = orc.GameLogic(cfg.rules, cfg.n)
    w = rollout_workload(name)
    out = {}
    for count in (w.G, 65, 1):
        states = w.states if count == w.G else sub_batch(w, count)[0]
        out[count] = (states, count, _oracle_rollouts(cfg, lg, states, count, ROLLOUT_SEEDS, ROLLOUT_CAP, ROLLOUT_BASE))
    return out, win_reason_hist(out[w.G][2])


@functools.lru_cache(maxsize=None)
def advance_expectation(name):
    cfg = CONFIGS[name]
    w = rollout_workload(name)
    want = pu.clone_states(w.states, w.G)
    orc.batch_random_advance(orc.GameLogic(cfg.rules, cfg.n), want, w.G, cfg.wb, ADVANCE_SEED, advance_plies(w.G), ADVANCE_BASE)
    return want


def oracle_mcts(lg, states, G, wb, params, base, width=MCTS_WIDTH, workers=16):
    """orc.batch_mcts over slices of the batch side by side on host threads (the counters are sums over games): the same children, counts
    and statistics as one call."""
    with ThreadPoolExecutor(max_workers=workers) as ex:
        parts = list(ex.map(lambda job: orc.batch_mcts(lg, job[1], len(job[1]), wb, params, base + job[0], width), _slices(states, G, workers)))
    kids = (TaflRootChild * (G * width)).from_buffer_copy(b"".join(bytes(p[0]) for p in parts))
    cnt = (C.c_uint32 * G)(*[c for p in parts for c in p[1]])
    stats = TaflMctsStats()
    for _, _, s in parts:
        for f in STAT_FIELDS:
            setattr(stats, f, getattr(stats, f) + getattr(s, f))
        for i in range(16):
            stats.reason_hist[i] += s.reason_hist[i]
    return kids, cnt, stats


def mcts_params(name, flags=0):
    return TaflMctsParams(mcts_sims(name), MCTS_CAP, MCTS_CPUCT, MCTS_SEED, 0, flags)


@functools.lru_cache(maxsize=None)
def mcts_expectation(name):
    cfg = CONFIGS[name]
    w, _, _ = mcts_workload(name)
    return oracle_mcts(orc.GameLogic(cfg.rules, cfg.n), w.states, w.G, cfg.wb, mcts_params(name), MCTS_BASE)


# ---- coverage conditions: on the oracle's output, never on an engine's -----------------------------------------------------------------

def check_rollout_coverage(name):
    """Check (a) of a preset board must see every rare outcome often enough; returns the oracle's histogram."""
    _, hist = rollout_expectations(name)
    for reason, floor in ROLLOUT_FLOORS.get(name, {}).items():
        assert hist[reason] >= floor, (name, abi.WIN_REASON_NAMES[reason], hist[reason], floor)
    return hist


def check_mcts_coverage(name):
    _, left_out, size = mcts_workload(name)
    assert left_out <= MCTS_MAX_LEFT_OUT * size, (name, left_out, size)
    _, _, stats = mcts_expectation(name)
    for key, floor in MCTS_FLOORS.get(name, {}).items():
        got = stats.terminal_hits if key == "terminal_hits" else stats.reason_hist[key]
        assert got >= floor, (name, key, got, floor)
    return stats


# ---- engine adapters ---------------------------------------------------------------------------------------------------------------------

class HostSimEngine:
    """The product's device code compiled for the host with run-time Consts (13x13 Copenhagen in the dense layout, as the library)."""
    label = "host-sim"

    def __init__(self, rules, n, wb):
        from tests.hostsim import hostsim
        self._hostsim = hostsim
        self.hs = hostsim.HostSim(rules, n, wb)
        self.dense13 = n == 13 and wb == 256 and bytes(rules.to_c()) == bytes(abi.rules.COPENHAGEN.to_c())
        self.pipelines = self.run_pipelines = (("host", 0),)

    def _dense(self, f):
        self._hostsim.set_dense13(self.dense13)
        try:
            return f()
        finally:
            self._hostsim.set_dense13(False)

    def rollout(self, states, G, seed, sim, cap, base):
        """(results, the batch afterwards)"""
        mine = pu.clone_states(states, G)
        return self._dense(lambda: self.hs.rollout(mine, G, seed, sim, cap, base)), mine

    def random_advance(self, states, G, seed, plies, base):
        mine = pu.clone_states(states, G)
        self._dense(lambda: self.hs.random_advance(mine, G, seed, plies, base))
        return mine

    def mcts(self, states, G, params, base, width):
        """(children, counts, stats, the batch afterwards)"""
        mine = pu.clone_states(states, G)
        return self._dense(lambda: self.hs.mcts(mine, G, params, base, width)) + (mine,)

    def selfplay(self, states, G, params, n_moves, base):
        """(plays [m * G + g], stats, the batch afterwards)"""
        mine = pu.clone_states(states, G)
        plays, stats = self._dense(lambda: self.hs.selfplay(mine, G, params, n_moves, base))
        return plays, stats, mine

    def record(self, states, G, params_at, pieces, base, sample_seed, temp_moves, max_moves, K):
        """The recording run in `pieces` [(moves, move_base)] into one examples object, then finalize: a Recording."""
        mine = pu.clone_states(states, G)
        hx = xu.HostExamples(self.hs.rules, self.hs.n, self.hs.wb, G, max_moves, K)
        rows, sims, faults = [], 0, 0
        xu.hlib().hsx_set_dense13(int(self.dense13))
        try:
            for n_piece, move_base in pieces:
                plays, stats = hx.record(mine, params_at(move_base), n_piece, base, sample_seed, temp_moves, move_base)
                rows += _play_rows(plays, n_piece, G)
                sims, faults = sims + stats.sims, faults + stats.faults
        finally:
            xu.hlib().hsx_set_dense13(0)
        hx.finalize(mine)
        lens, counters = hx.counts()
        return Recording(rows, mine, lens, hx.example, counters, sims, faults, None, lambda: None)

    def gmcts(self, states, G, S, c_puct, salts, edges):
        """(children per game, (sims, predicts, terminal_hits, faults), the dense getters or None)"""
        kids, counts, _ = gu.run_hostsim_guided(self.hs, self._hostsim.lib(), pu.clone_states(states, G), G, S, c_puct, salts, edges)
        return kids, counts, None

    def gselfplay(self, states, G, S, c_puct, salts, n_moves, sample_seed, temp_moves, base, edges):
        """(Run, examples per game, overflow marks, lens, counters, faults)"""
        ex = gsu.HostExamples(self.hs.n, G, n_moves, S)
        got, faults, _ = gsu.host_run(self.hs.rules, self.hs.n, self.hs.wb, pu.clone_states(states, G), S, c_puct, salts, n_moves, sample_seed, temp_moves,
                                      ex, base=base, edges_per_node=edges)
        examples, overflow = ex.all()
        lens, counters = ex.counts()
        return got, examples, overflow, lens, counters, sum(faults) + got.stat_faults

    def close(self):
        pass


class GpuEngine:
    """The library through the C-ABI: BatchedGameLogic / new_batch / upload (the preset kernels where the context detects a preset)."""
    label = "gpu"

    def __init__(self, rules, n, wb):
        from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
        self.logic = BatchedGameLogic(rules, n, wb)
        fused = wb == 64                # the fused kernel is the default of 64-bit boards; the other boards default to two kernels
        self.pipelines = (("default", 0), ("two-kernel", abi.mcts_tune(abi.MCTS_PIPELINE_TWO_KERNEL, 4 if fused else 1)))
        # default tuning against one playout slot per game (no speculation): the self-play runs (which have no fused form) and check (i),
        # whose kept statistics have no oracle, so that the one-slot run is the nearest thing to a reference.  On 64-bit boards the default
        # of a search is the fused kernel with two slots, of a run the two-kernel pipeline.
        self.run_pipelines = (("default", 0), ("two-kernel, one slot", abi.mcts_tune(abi.MCTS_PIPELINE_TWO_KERNEL, 1)))

    def _batch(self, states, G):
        b = self.logic.new_batch(G)
        b.upload(states)
        return b

    def rollout(self, states, G, seed, sim, cap, base):
        b = self._batch(states, G)
        try:
            return b.rollout(seed, sim, cap, base), b.download()
        finally:
            b.close()

    def random_advance(self, states, G, seed, plies, base):
        b = self._batch(states, G)
        try:
            b.random_advance(seed, plies, base)
            return b.download()
        finally:
            b.close()

    def mcts(self, states, G, params, base, width):
        b = self._batch(states, G)
        try:
            b.mcts_run(params.n_sims, params.c_puct, params.seed, params.max_rollout_plies, game_id_base=base, flags=params.flags)
            kids, cnt = b.mcts_root_children(width)
            return kids, cnt, b.mcts_stats(), b.download()
        finally:
            b.close()

    def selfplay(self, states, G, params, n_moves, base):
        b = self._batch(states, G)
        try:
            plays = b.selfplay_run(n_moves, params.n_sims, params.c_puct, params.seed, params.max_rollout_plies, game_id_base=base,
                                   sim_offset=params.sim_offset, flags=params.flags)
            return plays, b.mcts_stats(), b.download()
        finally:
            b.close()

    def record(self, states, G, params_at, pieces, base, sample_seed, temp_moves, max_moves, K):
        import numpy as np
        b = self._batch(states, G)
        ex = self.logic.new_examples(G, max_moves, K)
        try:
            rows, sims, faults = [], 0, 0
            for n_piece, move_base in pieces:
                p = params_at(move_base)
                plays = b.selfplay_record(ex, n_piece, p.n_sims, p.c_puct, p.seed, p.max_rollout_plies, game_id_base=base, sim_offset=p.sim_offset,
                                          flags=p.flags, sample_seed=sample_seed, temp_moves=temp_moves, move_base=move_base)
                rows += _play_rows(plays, n_piece, G)
                st = b.mcts_stats()
                sims, faults = sims + st.sims, faults + st.faults
            ex.finalize(b)
            after = b.download()
            lens, total = ex.counts()
            lens = list(lens)
            assert total == sum(lens) and max(lens, default=0) <= max_moves
            idx = np.array([j * G + g for g in range(G) for j in range(lens[g])], np.uint32)
            table = {}
            if idx.size:
                nc, ov, pl, mv, acts, vis = ex.read(idx)
                boards, sides, _pi, z, fin = ex.gather(idx)
                for i, e in enumerate(idx):
                    k = int(nc[i])
                    table[int(e)] = ((boards[i].tolist(), int(sides[i]), acts[i, :k].tolist(), vis[i, :k].tolist(), int(pl[i]), int(mv[i])),
                                     int(ov[i]), np.float32(z[i]), int(fin[i]))
            es = ex.stats()
        except BaseException:
            ex.close()
            raise
        finally:
            b.close()
        return Recording(rows, after, lens, lambda j, g: table[j * G + g], {"dropped": es.dropped, "overflowed": es.overflowed, "bad_index": es.bad_index},
                         sims, faults, ex.gather, ex.close)

    def gmcts(self, states, G, S, c_puct, salts, edges):
        b = self._batch(states, G)
        try:
            kids, st, _ = gu.run_device_guided(b, G, self.logic.side_len, S, c_puct, salts, edges)
            return kids, (st.sims, st.predicts, st.terminal_hits, st.faults), (b.gmcts_root_visits(), b.gmcts_policy(1.0))
        finally:
            b.close()

    def gselfplay(self, states, G, S, c_puct, salts, n_moves, sample_seed, temp_moves, base, edges):
        b = self._batch(states, G)
        ex = self.logic.new_examples(G, n_moves, S)
        try:
            got, overflow, st = gsu.device_run(b, ex, self.logic.side_len, S, c_puct, salts, n_moves, sample_seed, temp_moves, base=base, edges_per_node=edges)
            es = ex.stats()
            return (got, got.examples, overflow, list(ex.counts()[0]), {"dropped": es.dropped, "overflowed": es.overflowed, "bad_index": es.bad_index},
                    st.faults)
        finally:
            ex.close()
            b.close()

    def mcts_advance(self, states, G, params, base, width):
        """mcts_run, mcts_advance(None), then a keep-search of as many simulations again:
        (plays, effects, the batch after the advance, tree nodes per game, the keep-search's root children, its faults)"""
        b = self._batch(states, G)
        try:
            b.mcts_run(params.n_sims, params.c_puct, params.seed, params.max_rollout_plies, game_id_base=base, flags=params.flags)
            plays, eff = b.mcts_advance(None)
            after, nodes = b.download(), list(b.mcts_tree_nodes())
            b.mcts_run(params.n_sims, params.c_puct, params.seed, params.max_rollout_plies, game_id_base=base, flags=params.flags, keep=True)
            kids, cnt = b.mcts_root_children(width)
            rec, cnt = pu.children_view(kids, cnt, G, width)
            return plays, eff, after, nodes, [pu.children_of(rec, cnt, g) for g in range(G)], b.mcts_stats().faults
        finally:
            b.close()

    def gmcts_advance(self, states, G, S, c_puct, salts, edges):
        """(plays, effects, the batch after the advance, guided tree nodes per game, the stats of a keep-search of S more simulations)"""
        b = self._batch(states, G)
        try:
            gu.run_device_guided(b, G, self.logic.side_len, S, c_puct, salts, edges)
            plays, eff = b.gmcts_advance(None)
            after, nodes = b.download(), list(b.gmcts_tree_nodes())
            _, st, _ = gu.run_device_guided(b, G, self.logic.side_len, S, c_puct, salts, edges, keep=True)
            return plays, eff, after, nodes, st
        finally:
            b.close()

    def close(self):
        self.logic.close()


# ---- comparisons -------------------------------------------------------------------------------------------------------------------------

def _compare_rollouts(engine, cfg, states, G, want, cap, base, tag):
    for seed, tuples in want.items():
        got, after = engine.rollout(states, G, seed, ROLLOUT_SIM, cap, base)
        for g in range(G):
            if result_tuple(got[g]) != tuples[g]:
                raise AssertionError(f"{engine.label} {tag} seed {seed} game {g} of {G}: oracle {tuples[g]}, engine {result_tuple(got[g])} "
                                     f"(value, status, reason, winner, plies)\n{pu.describe_state(states[g], cfg.wb)}")
        assert pu.states_equal(states, after, G), f"{engine.label} {tag} seed {seed}: a rollout must not modify the batch " \
                                                  f"(game {pu.first_state_diff(states, after, G)})"


def compare_rollouts(engine, name):
    """Check (a)."""
    cfg = CONFIGS[name]
    batches, _ = rollout_expectations(name)
    for count, (states, G, want) in batches.items():
        _compare_rollouts(engine, cfg, states, G, want, ROLLOUT_CAP, ROLLOUT_BASE, f"{name} rollout")


def compare_advance(engine, name):
    """Check (b)."""
    cfg = CONFIGS[name]
    w = rollout_workload(name)
    want = advance_expectation(name)
    got = engine.random_advance(w.states, w.G, ADVANCE_SEED, advance_plies(w.G), ADVANCE_BASE)
    g = pu.first_state_diff(want, got, w.G)
    if g >= 0:
        raise AssertionError(f"{engine.label} {name} random_advance: game {g} ({kind_of(w, g)}, {g % 7 + 1} plies) from\n"
                             f"{pu.describe_state(w.states[g], cfg.wb)}\noracle\n{pu.describe_state(want[g], cfg.wb)}\n"
                             f"engine\n{pu.describe_state(got[g], cfg.wb)}")


def compare_hint(make_engine, n, wb):
    """Check (c); `make_engine(rules, n, wb)` builds the adapter of one ruleset."""
    w, multi = hint_workload(n, wb)
    assert multi >= 20, (n, multi)
    for label, rules in hint_rules():
        cfg = Config(f"shieldwall {label} {n}x{n}", rules, n, wb, label == "preset")
        want = _oracle_rollouts(cfg, orc.GameLogic(rules, n), w.states, w.G, HINT_SEEDS, HINT_CAP, ROLLOUT_BASE)
        engine = make_engine(rules, n, wb)
        try:
            _compare_rollouts(engine, cfg, w.states, w.G, want, HINT_CAP, ROLLOUT_BASE, cfg.name)
        finally:
            engine.close()


def compare_mcts(engine, name):
    """Check (d), once per pipeline of the engine."""
    cfg = CONFIGS[name]
    w, _, _ = mcts_workload(name)
    ok, on, ostats = mcts_expectation(name)
    orec, ocnt = pu.children_view(ok, on, w.G, MCTS_WIDTH)
    for label, flags in engine.pipelines:
        tag = f"{engine.label} {name} mcts ({label})"
        gk, gn, gstats, after = engine.mcts(w.states, w.G, mcts_params(name, flags), MCTS_BASE, MCTS_WIDTH)
        grec, gcnt = pu.children_view(gk, gn, w.G, MCTS_WIDTH)
        g = pu.first_children_diff(orec, ocnt, grec, gcnt)
        if g >= 0:
            raise AssertionError(f"{tag}: root children of game {g} ({kind_of(w, g)})\n{pu.describe_state(w.states[g], cfg.wb)}\n"
                                 f"oracle {pu.children_of(orec, ocnt, g)}\nengine {pu.children_of(grec, gcnt, g)}")
        for f in STAT_FIELDS:
            assert getattr(ostats, f) == getattr(gstats, f), (tag, f, getattr(ostats, f), getattr(gstats, f))
        assert list(ostats.reason_hist) == list(gstats.reason_hist), (tag, list(ostats.reason_hist), list(gstats.reason_hist))
        assert pu.states_equal(w.states, after, w.G), f"{tag}: a search must not modify the batch"


# ======== checks e .. i: the code that makes a move and goes on, from the crafted mix of check (d) ======================================

def run_moves(name):
    return 3 if CONFIGS[name].n == 13 else 4


def guided_sims(name):
    return 24 if CONFIGS[name].n == 13 else 32


def guided_moves(name):
    return 4 if CONFIGS[name].n == 7 else 3


def guided_salts(G):
    return [(3 * g + 1) % 256 for g in range(G)]


def run_params(name, sim_offset=0, flags=0):
    return TaflMctsParams(mcts_sims(name), MCTS_CAP, MCTS_CPUCT, MCTS_SEED, sim_offset, flags)


# ---- the oracle's runs (computed once per process, never modified) -----------------------------------------------------------------------

RecordWant = collections.namedtuple("RecordWant", "plays examples info states")       # plays [m][g], examples per game, info, final states


@functools.lru_cache(maxsize=None)
def record_expectation(name, temp_moves):
    """examples_util.oracle_record from the workload of check (d); temp_moves = 0 is also the expectation of the plain self-play run."""
    cfg = CONFIGS[name]
    w, _, _ = mcts_workload(name)
    states = pu.clone_states(w.states, w.G)
    plays, ex, info = xu.oracle_record(orc, orc.GameLogic(cfg.rules, cfg.n), states, w.G, cfg.wb, mcts_sims(name), MCTS_CAP, MCTS_CPUCT, MCTS_SEED,
                                       MCTS_BASE, run_moves(name), RUN_SSEED, temp_moves, workers=16)
    return RecordWant(plays, ex, info, states)


GuidedWant = collections.namedtuple("GuidedWant", "children plays counts")            # [(action, visits, q hex)] and TaflPlay per game; sums


@functools.lru_cache(maxsize=None)
def guided_expectation(name):
    """GameLogic.gmcts per game with the stub network; counts = (sims, predicts, terminal hits) summed over the oracle's own counters."""
    cfg = CONFIGS[name]
    w, _, _ = mcts_workload(name)
    lg, A, salts = orc.GameLogic(cfg.rules, cfg.n), abi.action_size(cfg.n), guided_salts(w.G)
    children, plays, counts = [], [], [0, 0, 0]
    for g in range(w.G):
        kids, _ns, _pri, cnt = lg.gmcts(orc.GameState.from_abi(w.states[g], cfg.wb), guided_sims(name), G_CPUCT,
                                        lambda s, g=g: gsu.stub(matrix_bytes_of(s.board_to_matrix()), int(s.side_to_play), A, salts[g]), cfg.wb)
        children.append([(a, v, float(q).hex()) for (_p, a, v, q) in kids])
        plays.append([p for (p, _a, _v, _q) in kids])
        for i in range(3):
            counts[i] += cnt[i]
    return GuidedWant(children, plays, tuple(counts))


@functools.lru_cache(maxsize=None)
def gselfplay_expectation(name):
    cfg = CONFIGS[name]
    w, _, _ = mcts_workload(name)
    return gsu.oracle_run(orc, orc.GameLogic(cfg.rules, cfg.n), w.states, cfg.wb, guided_sims(name), G_CPUCT, guided_salts(w.G), guided_moves(name),
                          RUN_SSEED, H_TEMP, base=MCTS_BASE)


def _state_of(raw):
    return raw if isinstance(raw, TaflState) else TaflState.from_buffer_copy(raw)


def ending_hist(final_states, moves_made):
    """(Counter of the win reasons of the games that ended inside a run, how many of them had made two moves or more) - every game of the
    workload is ONGOING at the start."""
    hist, later = collections.Counter(), 0
    for raw, made in zip(final_states, moves_made):
        st = _state_of(raw)
        if st.status != abi.ONGOING:
            later += made >= 2
            if st.status == abi.WIN:
                hist[st.reason] += 1
    return hist, later


def record_endings(want):
    return ending_hist([want.states[g] for g in range(len(want.examples))], [len(e) for e in want.examples])


# ---- coverage conditions of the runs: on the oracle's output, never on an engine's -------------------------------------------------------

def _check_floors(tag, hist, later, floors):
    for key, floor in floors.items():
        got = later if key == "later" else hist[key]
        assert got >= floor, (tag, key if key == "later" else abi.WIN_REASON_NAMES[key], got, floor)


def check_left_out(name):
    """Roots without a legal play while ONGOING are left out of the workload of checks (d) .. (i): at most MCTS_MAX_LEFT_OUT of the list."""
    _, left_out, size = mcts_workload(name)
    assert left_out <= MCTS_MAX_LEFT_OUT * size, (name, left_out, size)


def check_run_coverage(name, temp_moves=0):
    """Checks (e) and (f): rare endings inside the run, later endings, no overflow at K = 64, and a sampled run that leaves the argmax."""
    check_left_out(name)
    want = record_expectation(name, temp_moves)
    assert want.info["widest"] < RUN_K, (name, want.info)
    assert want.info["searches"] == want.info["game_moves"], (name, want.info)          # every search of a live game makes a move
    if temp_moves:
        assert 4 * want.info["non_argmax"] >= want.info["game_moves"], (name, want.info)
    else:
        assert want.info["non_argmax"] == 0
    hist, later = record_endings(want)
    _check_floors((name, temp_moves), hist, later, (RUN_FLOORS_SAMPLED if temp_moves else RUN_FLOORS)[name])
    return hist, later


def check_guided_coverage(name):
    check_left_out(name)
    want = guided_expectation(name)
    assert want.counts[2] >= GUIDED_HIT_FLOORS[name], (name, want.counts)
    return want.counts


def check_gselfplay_coverage(name):
    check_left_out(name)
    want = gselfplay_expectation(name)
    hist, later = ending_hist(want.states, want.moves)
    _check_floors((name, "guided"), hist, later, GSELFPLAY_FLOORS[name])
    return hist, later


# ---- comparisons --------------------------------------------------------------------------------------------------------------------------

def _play_rows(plays, n_moves, G):
    return [[pu.play_tuple4(plays[m * G + g]) for g in range(G)] for m in range(n_moves)]


def _same_plays_and_states(tag, cfg, w, got_rows, want_rows, got_states, want_states, G, ids=None):
    for m, (a, b) in enumerate(zip(got_rows, want_rows)):
        for g in range(G):
            assert a[g] == b[g], f"{tag}: move {m} of game {ids[g] if ids else g} ({kind_of(w, ids[g] if ids else g)}): oracle {b[g]}, engine {a[g]}\n" \
                                 f"{pu.describe_state(w.states[ids[g] if ids else g], cfg.wb)}"
    g = pu.first_state_diff(want_states, got_states, G)
    if g >= 0:
        raise AssertionError(f"{tag}: final state of game {ids[g] if ids else g}\noracle\n{pu.describe_state(want_states[g], cfg.wb)}\n"
                             f"engine\n{pu.describe_state(got_states[g], cfg.wb)}")


def first_rare_ending(want):
    """The first game that the oracle's run ended by enclosure, exit fort, all captured or no plays."""
    for g in range(len(want.examples)):
        st = want.states[g]
        if st.status == abi.WIN and st.reason in RARE_REASONS:
            return g
    raise AssertionError("no game ended by a rare rule")


def compare_selfplay(engine, name):
    """Check (e): the self-play run against the oracle loop with temp_moves = 0, once per pipeline, then the first rare-rule game alone
    under its global id (a batch whose only wave has one live lane)."""
    cfg = CONFIGS[name]
    w, _, _ = mcts_workload(name)
    want = record_expectation(name, 0)
    n_moves, sims = run_moves(name), mcts_sims(name)
    for label, flags in engine.run_pipelines:
        tag = f"{engine.label} {name} selfplay ({label})"
        plays, stats, after = engine.selfplay(w.states, w.G, run_params(name, 0, flags), n_moves, MCTS_BASE)
        _same_plays_and_states(tag, cfg, w, _play_rows(plays, n_moves, w.G), want.plays, after, want.states, w.G)
        # `sims` is what pins the stop of a game that has ended (selfplay_advance_impl's test of the status after the play): a search started
        # from a terminal root yields no play, so plays and states stay the same and only this counter shows the searches that should not run
        assert stats.sims == want.info["searches"] * sims and stats.faults == 0, (tag, stats.sims, want.info["searches"] * sims, stats.faults)
    g = first_rare_ending(want)
    one = pu.states_array([w.states[g]])
    plays, stats, after = engine.selfplay(one, 1, run_params(name), n_moves, MCTS_BASE + g)
    _same_plays_and_states(f"{engine.label} {name} selfplay (one game)", cfg, w, _play_rows(plays, n_moves, 1), [[row[g]] for row in want.plays], after,
                           pu.states_array([want.states[g]]), 1, ids=[g])
    assert stats.sims == len(want.examples[g]) * sims and stats.faults == 0, (name, g, stats.sims, stats.faults)


def record_cases(name):
    """(temp_moves, [(moves of the piece, move_base)]): all argmax, all sampled, and the sampled run in two pieces."""
    n = run_moves(name)
    return ((0, ((n, 0),)), (n, ((n, 0),)), (n, ((2, 0), (n - 2, 2))))


def compare_record(engine, name):
    """Check (f): the recording run against examples_util.oracle_record - plays, states, lens, every example field, z and final after
    finalize, the counters - and, where the engine gathers on the device, the examples of the ended games under all eight symmetries."""
    cfg = CONFIGS[name]
    w, _, _ = mcts_workload(name)
    n_moves, sims = run_moves(name), mcts_sims(name)
    for temp_moves, pieces in record_cases(name):
        want = record_expectation(name, temp_moves)
        assert want.info["widest"] < RUN_K
        tag = f"{engine.label} {name} record (temp_moves {temp_moves}, {len(pieces)} piece(s))"
        rec = engine.record(w.states, w.G, lambda move_base: run_params(name, move_base * sims), pieces, MCTS_BASE, RUN_SSEED, temp_moves, n_moves, RUN_K)
        try:
            _same_plays_and_states(tag, cfg, w, rec.plays, want.plays, rec.states, want.states, w.G)
            # `sims` is what pins the stop of a game that has ended inside a run (see compare_selfplay).  A game that is over when a run BEGINS
            # is searched once from its terminal root (include/taflhip.h tafl_selfplay_run: n_sims terminal hits, as tafl_mcts_run and the
            # oracle's batch_mcts book them), hence the term for the later pieces, counted on the oracle's states and lens
            over = sum(1 for _n, move_base in pieces[1:] for g in range(w.G) if want.states[g].status != abi.ONGOING and len(want.examples[g]) <= move_base)
            assert rec.sims == (want.info["searches"] + over) * sims and rec.faults == 0, (tag, rec.sims, want.info["searches"], over, sims, rec.faults)
            assert rec.counters == {"dropped": 0, "overflowed": 0, "bad_index": 0}, (tag, rec.counters)
            xu.check_examples(rec.example, rec.lens, want.examples, w.G, tag)
            if rec.gather is not None:
                _compare_gather(rec, cfg, want, w.G, tag)
        finally:
            rec.close()


def _compare_gather(rec, cfg, want, G, tag):
    import numpy as np
    rows = [(j, g, s, e) for g in range(G) if want.states[g].status != abi.ONGOING for j, e in enumerate(want.examples[g]) for s in range(8)]
    assert rows, tag
    boards, sides, pi, z, fin = rec.gather([j * G + g for j, g, _, _ in rows], [s for _, _, s, _ in rows])
    for i, (j, g, s, e) in enumerate(rows):
        assert np.array_equal(pi[i], xu.dense_pi(cfg.n, e, s)), (tag, "pi", g, j, s)
        assert np.array_equal(boards[i], xu.sym_board_np(np.array(e.board, np.uint8), s)), (tag, "board", g, j, s)
        assert (sides[i], z[i], fin[i]) == (e.side, e.z, e.final) and e.final == 1, (tag, g, j, s, sides[i], z[i], fin[i], e.side, e.z, e.final)


def compare_guided(engine, name):
    """Check (g): one guided search per game against GameLogic.gmcts; where the engine has them, the dense getters against the children."""
    cfg = CONFIGS[name]
    w, _, _ = mcts_workload(name)
    want = guided_expectation(name)
    S, A = guided_sims(name), abi.action_size(cfg.n)
    kids, counts, dense = engine.gmcts(w.states, w.G, S, G_CPUCT, guided_salts(w.G), G_EDGES)
    tag = f"{engine.label} {name} guided search"
    for g in range(w.G):
        assert kids[g] == want.children[g], f"{tag}: root children of game {g} ({kind_of(w, g)})\n{pu.describe_state(w.states[g], cfg.wb)}\n" \
                                            f"oracle {want.children[g]}\nengine {kids[g]}"
    assert tuple(counts) == want.counts + (0,), (tag, "sims, predicts, terminal_hits, faults", tuple(counts), want.counts)
    if dense is not None:
        visits, policy = dense
        for g in range(w.G):
            vs = {a: v for a, v, _ in want.children[g]}
            N = float(sum(vs.values()))
            assert {a: visits[g * A + a] for a in range(A) if visits[g * A + a]} == vs, (tag, "root_visits", g)
            if N:
                assert {a: policy[g * A + a] for a in range(A) if policy[g * A + a] != 0} == {a: v / N for a, v in vs.items()}, (tag, "policy", g)


def compare_gselfplay(engine, name):
    """Check (h): guided self-play at each game's own pace against gselfplay_util.oracle_run."""
    cfg = CONFIGS[name]
    w, _, _ = mcts_workload(name)
    want = gselfplay_expectation(name)
    tag = f"{engine.label} {name} guided self-play"
    got, examples, overflow, lens, counters, faults = engine.gselfplay(w.states, w.G, guided_sims(name), G_CPUCT, guided_salts(w.G), guided_moves(name),
                                                                       RUN_SSEED, H_TEMP, MCTS_BASE, G_EDGES)
    gsu.assert_same_run(got, want, examples, where=tag)
    assert got.sims == want.sims and faults == 0, (tag, got.sims, want.sims, faults)
    assert lens == want.moves and counters == {"dropped": 0, "overflowed": 0, "bad_index": 0} and not any(any(o) for o in overflow), (tag, counters)


def _first_max(children):
    vs = [v for _a, v, _q in children]
    return vs.index(max(vs))


def _oracle_step(cfg, w, plays):
    """(effects tuples, states) of orc.batch_step of one play per game from the workload."""
    states = pu.clone_states(w.states, w.G)
    sub = (TaflPlay * w.G)()
    for g, p in enumerate(plays):
        C.memmove(C.byref(sub[g]), C.byref(p), C.sizeof(TaflPlay))
    eff = orc.batch_step(orc.GameLogic(cfg.rules, cfg.n), states, w.G, cfg.wb, sub)
    return [pu.effects_tuple(eff[g]) for g in range(w.G)], states, [pu.play_tuple4(p) for p in plays]


def _same_advance(tag, cfg, w, got, want):
    (plays, eff, after), (weff, wstates, wplays) = got, want
    for g in range(w.G):
        assert pu.play_tuple4(plays[g]) == wplays[g], f"{tag}: play of game {g}: oracle {wplays[g]}, engine {pu.play_tuple4(plays[g])}"
        assert pu.effects_tuple(eff[g]) == weff[g], f"{tag}: effects of game {g} ({kind_of(w, g)}): oracle {weff[g]}, engine {pu.effects_tuple(eff[g])}\n" \
                                                    f"{pu.describe_state(w.states[g], cfg.wb)}"
    g = pu.first_state_diff(wstates, after, w.G)
    assert g < 0, f"{tag}: state of game {g}\noracle\n{pu.describe_state(wstates[g], cfg.wb)}\nengine\n{pu.describe_state(after[g], cfg.wb)}"


@functools.lru_cache(maxsize=None)
def advance_expectation_mcts(name):
    """orc.batch_step of the oracle's first-maximum root child of check (d)'s search; also the histogram of the children's endings."""
    cfg = CONFIGS[name]
    w, _, _ = mcts_workload(name)
    ok, on, _ = mcts_expectation(name)
    rec, cnt = pu.children_view(ok, on, w.G, MCTS_WIDTH)
    plays = []
    for g in range(w.G):
        vs = [int(v) for v in rec["visits"][g, :int(cnt[g])]]
        plays.append(TaflPlay.from_buffer_copy(int(rec["play"][g, vs.index(max(vs))]).to_bytes(4, "little")))
    return _oracle_step(cfg, w, plays)


@functools.lru_cache(maxsize=None)
def advance_expectation_guided(name):
    cfg = CONFIGS[name]
    w, _, _ = mcts_workload(name)
    want = guided_expectation(name)
    return _oracle_step(cfg, w, [want.plays[g][_first_max(want.children[g])] for g in range(w.G)])


def check_advance_coverage(name, kind, want):
    """The children that the advance is driven onto: terminal ones by a rare rule, and captures of two pieces or more."""
    check_left_out(name)
    weff, wstates, _ = want
    rare = sum(1 for g in range(len(weff)) if wstates[g].status == abi.WIN and wstates[g].reason in RARE_REASONS)
    multi = sum(1 for e in weff if e[5] >= 2)
    floor = ADVANCE_FLOORS[name][kind]
    assert rare >= floor[0] and multi >= floor[1], (name, kind, rare, multi, floor)
    return rare, multi


def compare_advance_onto_children(engine, name):
    """Check (i), device only: advance(None) after check (d)'s search against the oracle's step of the first-maximum child; a tree stays for
    every game; a keep-search of S more simulations gives the same children - each step under the default tuning (the fused kernel on 64-bit
    boards, the two-kernel pipeline elsewhere) and under mcts_tune(TWO_KERNEL, slots=1).  Then the guided tree after check (g)'s
    search against the oracle's do_play (batch_step) of its first-maximum child."""
    cfg = CONFIGS[name]
    w, _, _ = mcts_workload(name)
    want = advance_expectation_mcts(name)
    assert all(e[1] == 0 for e in want[0]), name                  # the oracle accepts every play
    check_advance_coverage(name, "mcts", want)
    kept = []
    for label, flags in engine.run_pipelines:
        tag = f"{engine.label} {name} mcts_advance ({label})"
        plays, eff, after, nodes, kids, faults = engine.mcts_advance(w.states, w.G, mcts_params(name, flags), MCTS_BASE, MCTS_WIDTH)
        _same_advance(tag, cfg, w, (plays, eff, after), want)
        assert min(nodes) >= 1 and faults == 0, (tag, min(nodes), faults)
        kept.append(kids)
    assert all(k == kept[0] for k in kept[1:]), f"{engine.label} {name}: the keep-search after the advance depends on the tuning"
    want = advance_expectation_guided(name)
    check_advance_coverage(name, "guided", want)
    tag = f"{engine.label} {name} gmcts_advance"
    plays, eff, after, nodes, stats = engine.gmcts_advance(w.states, w.G, guided_sims(name), G_CPUCT, guided_salts(w.G), G_EDGES)
    _same_advance(tag, cfg, w, (plays, eff, after), want)
    assert min(nodes) >= 1 and stats.faults == 0, (tag, min(nodes), stats.faults)
