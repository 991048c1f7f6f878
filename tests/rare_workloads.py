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
"""
import collections
import ctypes as C
import functools
import random
from concurrent.futures import ThreadPoolExecutor

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflMctsParams, TaflMctsStats, TaflRootChild, TaflState
from oracle import oracle as orc
from tests import parity_util as pu

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
        self.pipelines = (("host", 0),)

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
