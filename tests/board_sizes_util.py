"""Workloads, oracle expectations and coverage floors for the tests at every board size (tests/test_hostsim_board_sizes.py,
tests/test_gpu_board_sizes.py).

tafl_ctx_create accepts a side length from 3 up to the row width of the board word: 3..7 on 64 bits, 3..11 on 128, 3..15 on 256 - the 27
pairs of ALL_PAIRS.  EDGE_PAIRS are the pairs at which something changes: both sides of the dense13 boundary (12, 13 | 14, 15 @256), a
board without a padding column on the 8-limb layout (15 @256), with one (14 @256, 10 @128, 6 @64), an even side (8 @128) and the tiny boards
(5, 4, 3 @64) whose action masks are shorter than the waves that count them.

Every expectation here comes from the oracle; the coverage floors are counted on the oracle's results alone and asserted before an engine
is compared.  The module itself uses no GPU (the device helpers gpu_logic / gpu_batch / expand_compare_gpu import the engine when called).

Crafted generators (tests/parity_util.py) and the smallest side at which they produce positions (CRAFTED_MIN, checked by
test_hostsim_board_sizes.py::test_crafted_generators_lower_bounds): sparse endgames from 3; enclosures from 5 (a ring needs an inner
tile and a tile outside it); shieldwalls from 6 (a wall of four, its two brackets); exit forts from 6 (the tallest seed shape spans six
rows and five columns).  Below its bound a generator raises or never returns; the lists leave it out there, explicitly.

Under KING_ENTRY throne movement (Copenhagen, Brandubh) the oracle never returns MOVE_THROUGH_BLOCKED_TILE: only NO_PASS and KING_PASS
test the tiles between (tafl_oracle.c validate_play_for_side).  The floor on that code is therefore met on a fifth ruleset, Copenhagen with
KING_PASS ("copenhagen_kingpass"), which runs the throne plays only; Copenhagen and Brandubh themselves must give none.

What the oracle gives per pair of EDGE_PAIRS (captures, captures on column 0 / n-1, leak positions, king captures over the four rulesets;
throne plays rejected ONTO under Copenhagen + Brandubh, THROUGH under copenhagen_kingpass) is written down next to TINY_COVERAGE below.
"""
import collections
import ctypes as C
import functools
import random

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflPlay, TaflState
from oracle import oracle as orc
from tests import parity_util as pu
from tests.training_rows_util import COPENHAGEN15, _fen_of

ALL_PAIRS = tuple((n, wb) for wb, top in ((64, 7), (128, 11), (256, 15)) for n in range(3, top + 1))
EDGE_PAIRS = ((15, 256), (14, 256), (13, 256), (12, 256), (10, 128), (6, 64), (8, 128), (5, 64), (4, 64), (3, 64))
FLOOR_PAIRS = tuple(p for p in EDGE_PAIRS if p[0] >= 6)          # the pairs the minimums of the floors apply to
RULE_LABELS = ("copenhagen", "brandubh", "rand0", "rand1")
CRAFTED_MIN = {"sparse": 3, "enclosure": 5, "shieldwall": 6, "exit_fort": 6}

# minimums per pair of FLOOR_PAIRS, over the four rulesets
FLOORS = {"captures": 20, "edge_captures": 20, "leak": 10, "king_captures": 5, "throne_onto": 5, "throne_through": 5}
FLOORS_BIG_COPENHAGEN = {"exit_forts": 5, "enclosure_wins": 5, "shieldwall_captures": 5}      # 14 and 15 @256 under Copenhagen


def pair_id(pair):
    return f"{pair[0]}@{pair[1]}"


# ---- start positions --------------------------------------------------------------------------------------------------------------------

def start_cells(n):
    """{(row, col): 'K' | 'T' | 't'}: the king on (n/2, n/2), defenders on the tiles within Manhattan distance 1 (2 from side 9 on) of it
    that lie off the edges, attackers on the middle of every edge (one tile below side 7, three below 11, five from 11 on) and, from side
    9 on, one more in front of each edge group."""
    c, m = n // 2, n - 1
    cells = {(c, c): "K"}
    reach = 2 if n >= 9 else 1
    half = 0 if n < 7 else (1 if n < 11 else 2)
    att = set()
    for d in range(-half, half + 1):
        att |= {(0, c + d), (m, c + d), (c + d, 0), (c + d, m)}
    if n >= 9:
        att |= {(1, c), (m - 1, c), (c, 1), (c, m - 1)}
    for r in range(1, m):
        for q in range(1, m):
            if 0 < abs(r - c) + abs(q - c) <= reach and (r, q) not in att:
                cells[(r, q)] = "T"
    for t in att:
        if t != (c, c):
            cells[t] = "t"
    return cells


def start_fen(n):
    """A start position for any side 3..15 (the literal Copenhagen 15 x 15 start of the training-row tests at 15)."""
    if not 3 <= n <= 15:
        raise ValueError("side length 3..15")
    return COPENHAGEN15 if n == 15 else _fen_of(n, start_cells(n))


# (attackers, defenders with the king) of start_fen(n), counted by hand from the rule above
START_COUNTS = {3: (4, 1), 4: (4, 3), 5: (4, 5), 6: (4, 5), 7: (12, 5), 8: (12, 5), 9: (16, 13), 10: (16, 13), 11: (24, 13), 12: (24, 13),
                13: (24, 13), 14: (24, 13), 15: (24, 13)}


# ---- rulesets ---------------------------------------------------------------------------------------------------------------------------

def rulesets(pair):
    """[(label, Ruleset)]: the Copenhagen and Brandubh presets and two random draws with seeds fixed per pair."""
    n, wb = pair
    return [("copenhagen", abi.rules.COPENHAGEN), ("brandubh", abi.rules.BRANDUBH),
            ("rand0", pu.random_ruleset(random.Random(7000 + 100 * n + wb))), ("rand1", pu.random_ruleset(random.Random(9000 + 100 * n + wb)))]


def ruleset(pair, label):
    if label == "copenhagen_kingpass":
        return abi.rules.COPENHAGEN.replace(throne_movement=abi.KING_PASS)
    return dict(rulesets(pair))[label]


# ---- positions --------------------------------------------------------------------------------------------------------------------------

def position_counts(n):
    """Positions per kind in the every-legal-play lists, by side: sized so that the oracle alone meets the floors and a case stays within
    a few seconds (a 15 x 15 position has some 150 legal plays, a 6 x 6 one some 20)."""
    if n >= 12:
        return {"random": 25, "enclosure": 12, "shieldwall": 36, "sparse": 25, "exit_fort": 12}
    if n >= 8:
        return {"random": 40, "enclosure": 16, "shieldwall": 36, "sparse": 40, "exit_fort": 16}
    return {"random": 80, "enclosure": 30, "shieldwall": 40, "sparse": 80, "exit_fort": 20}


@functools.lru_cache(maxsize=None)
def positions(pair):
    """[(kind, [TaflState])] of a pair: synthetic boards and every crafted kind whose lower bound the side meets (CRAFTED_MIN)."""
    n, wb = pair
    rng = random.Random(300 + 100 * n + wb)
    cnt = position_counts(n)
    arr = pu.random_board_states(rng, n, wb, cnt["random"])
    kinds = [("random", [arr[i] for i in range(cnt["random"])])]
    gens = {"enclosure": pu.enclosure_positions, "shieldwall": pu.shieldwall_positions, "sparse": pu.sparse_endgame_positions,
            "exit_fort": pu.exit_fort_positions}
    for kind in ("enclosure", "shieldwall", "sparse", "exit_fort"):
        if n >= CRAFTED_MIN[kind]:
            kinds.append((kind, gens[kind](rng, n, wb, cnt[kind])))
    return kinds


def position_list(pair):
    return [s for _k, lst in positions(pair) for s in lst]


def kind_spans(pair):
    out, at = {}, 0
    for kind, lst in positions(pair):
        out[kind] = (at, at + len(lst))
        at += len(lst)
    return out


def tiles_of(st, wb):
    """({attacker tiles}, {defender tiles, the king among them}) of an ABI state."""
    rw = abi.row_width(wb)
    a, d = abi.state_words(st, wb)
    body = (1 << (wb - 4)) - 1
    out = []
    for w in (a & body, d & body):
        s = set()
        while w:
            i = (w & -w).bit_length() - 1
            s.add((i // rw, i % rw))
            w &= w - 1
        out.append(s)
    return out


def throne_workload(pair, count=24):
    """(states, plays): a lone soldier of the side to move on the throne's row or column with nothing between, the king far away, and the
    play that lands ON the throne (even games) or passes THROUGH it to the tile behind (odd games)."""
    n, wb = pair
    c = n // 2
    rng = random.Random(500 + 100 * n + wb)
    states, plays = [], (TaflPlay * count)()
    for g in range(count):
        b = pu._blank(n, wb)
        side = (abi.ATTACKER, abi.DEFENDER)[(g // 2) % 2]
        k = rng.randrange(4)                                    # the piece left of, right of, above or below the throne
        dist = rng.randrange(1, c + 1) if k in (0, 2) else rng.randrange(1, n - c)
        tile = {0: (c, c - dist), 1: (c, c + dist), 2: (c - dist, c), 3: (c + dist, c)}[k]
        step = dist if g % 2 == 0 else dist + 1                 # onto / one past the throne (c - 1 and c + 1 are on every board)
        sign = 1 if k in (0, 2) else -1
        b["att" if side == abi.ATTACKER else "def"].add(tile)
        corners = ((0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1))
        off_lines = [(r, q) for r in range(n) for q in range(n) if r != c and q != c]
        free = [t for t in off_lines if t not in corners] or off_lines       # (side 3: the corners are all there is)
        b["king"] = rng.choice(free)
        b["att"].add(rng.choice([t for t in free if t != b["king"]]))
        states.append(pu._to_state(b, side))
        plays[g] = TaflPlay(tile[0], tile[1], abi.HORIZONTAL if k < 2 else abi.VERTICAL, sign * step)
    return pu.states_array(states), plays, count


# ---- the oracle's side (computed once per process, never modified) ----------------------------------------------------------------------

Expansion = collections.namedtuple("Expansion", "states G counts masks arr ranks total src plays effects after")


@functools.lru_cache(maxsize=None)
def oracle_expansion(pair, label):
    """Every legal play of every position of the pair under the ruleset, by the oracle."""
    n, wb = pair
    lg = orc.GameLogic(ruleset(pair, label), n)
    lst = position_list(pair)
    G = len(lst)
    states = pu.states_array(lst)
    oc, om = orc.batch_movegen(lg, states, G, wb)
    arr, ranks, total, src = pu.expand_all(states, G, oc)
    after = pu.clone_states(arr, total)
    op, oe = orc.batch_step_kth(lg, after, total, wb, ranks)
    return Expansion(states, G, oc, om, arr, ranks, total, src, op, oe, after)


def _capture_tiles(eff, rw):
    out = []
    for limb in range(abi.MAX_LIMBS):
        v = int(eff.captures[limb])
        while v:
            bit = limb * 64 + (v & -v).bit_length() - 1
            out.append((bit // rw, bit % rw))
            v &= v - 1
    return out


def _has_play_from(mask, base, n, tile):
    per = 2 * (n - 1)
    a0 = (tile[0] * n + tile[1]) * per
    return any((mask[base + (a >> 5)] >> (a & 31)) & 1 for a in range(a0, a0 + per))


@functools.lru_cache(maxsize=None)
def coverage(pair):
    """What the oracle's results hold, per pair over the four rulesets (+ per ruleset the big-board counters of Copenhagen)."""
    n, wb = pair
    rw, mw = abi.row_width(wb), (abi.action_size(n) + 31) // 32
    cov = collections.Counter()
    spans = kind_spans(pair)
    for label, rules in rulesets(pair):
        x = oracle_expansion(pair, label)
        lg = orc.GameLogic(rules, n)
        for i in range(x.total):
            e, p = x.effects[i], x.plays[i]
            if e.status == abi.WIN:
                cov[(label, abi.WIN_REASON_NAMES[e.reason])] += 1
                cov["king_captures"] += e.reason == abi.KING_CAPTURED
            if e.n_captures:
                cov["captures"] += 1
                to = abi.play_to(p)
                caps = _capture_tiles(e, rw)
                if p.from_col in (0, n - 1) or to[1] in (0, n - 1) or any(q in (0, n - 1) for _r, q in caps):
                    cov["edge_captures"] += 1
                if label == "copenhagen" and len(caps) >= 2 and "shieldwall" in spans and spans["shieldwall"][0] <= x.src[i] < spans["shieldwall"][1]:
                    wall = lg.detect_shieldwall(p, orc.GameState.from_abi(x.arr[i], wb))
                    cov["shieldwall_captures"] += bool(wall)
        for g in range(x.G):
            att, deff = tiles_of(x.states[g], wb)
            occ = att | deff
            for r in range(n - 1):
                if (r, n - 1) in occ and (r + 1, 0) in occ and (_has_play_from(x.masks, g * mw, n, (r, n - 1)) or _has_play_from(x.masks, g * mw, n, (r + 1, 0))):
                    cov["leak"] += 1
                    break
    cov["exit_forts"] = cov[("copenhagen", "ExitFort")]
    cov["enclosure_wins"] = cov[("copenhagen", "Enclosed")]
    states, plays, G = throne_workload(pair)
    c = n // 2
    for label in ("copenhagen", "brandubh", "rand0", "rand1", "copenhagen_kingpass"):
        lg = orc.GameLogic(ruleset(pair, label), n)
        for g in range(G):
            code = lg.validate_play(plays[g], orc.GameState.from_abi(states[g], wb))
            cov[("throne", label, code)] += 1
            if label in ("copenhagen", "brandubh"):
                cov["throne_onto"] += code == abi.MOVE_ONTO_BLOCKED_TILE and abi.play_to(plays[g]) == (c, c)
                cov["throne_through_king_entry"] += code == abi.MOVE_THROUGH_BLOCKED_TILE
            if label == "copenhagen_kingpass":
                cov["throne_through"] += code == abi.MOVE_THROUGH_BLOCKED_TILE
    return cov


def check_floors(pair):
    """The floors, on the oracle's results alone; returns the counters."""
    cov = coverage(pair)
    if pair in FLOOR_PAIRS:
        for key, floor in FLOORS.items():
            assert cov[key] >= floor, (pair, key, cov[key], floor)
        assert cov["throne_through_king_entry"] == 0, pair       # unreachable under KING_ENTRY (module docstring)
        if pair in ((14, 256), (15, 256)):
            for key, floor in FLOORS_BIG_COPENHAGEN.items():
                assert cov[key] >= floor, (pair, key, cov[key], floor)
    else:
        for key, want in TINY_COVERAGE[pair].items():
            assert cov[key] == want, (pair, key, cov[key], want)
    return cov


# what the oracle shows on the tiny boards, written down (compared for equality: a change of a generator or of the oracle shows here)
TINY_COVERAGE = {
    (5, 64): {"captures": 913, "edge_captures": 433, "leak": 237, "king_captures": 158, "throne_onto": 24, "throne_through": 12, "enclosure_wins": 87},
    (4, 64): {"captures": 373, "edge_captures": 290, "leak": 188, "king_captures": 23, "throne_onto": 24, "throne_through": 12, "enclosure_wins": 11},
    (3, 64): {"captures": 129, "edge_captures": 129, "leak": 177, "king_captures": 16, "throne_onto": 24, "throne_through": 12, "enclosure_wins": 0},
}
# ... and on the pairs the floors apply to (positions, legal plays under Copenhagen; then the counters in the order captures, on column
# 0 / n-1, leak positions, king captures; under Copenhagen exit forts, enclosure wins, shieldwall captures; throne 24 ONTO / 12 THROUGH each):
#   15@256: 110, 14 091; 2 262, 375, 80, 71; 159, 246, 17        14@256: 110, 12 929; 2 585, 539, 80, 97; 140, 312, 13
#   13@256: 110, 11 081; 1 638, 297, 84, 71; 353, 114, 11        12@256: 110,  9 987; 1 848, 335, 84, 110; 150, 135, 17
#   10@128: 148, 10 206; 1 765, 425, 120, 37; 106, 118, 13        8@128: 148,  6 163;   862, 314, 105, 52; 137, 94, 9
#    6@64:  250,  5 593; 1 445, 669, 210, 194; 96, 187, 9


# ---- device helpers (moved here from tests/test_gpu_parity.py, which imports them) ---------------------------------------------------------

_LOGICS = {}


def gpu_logic(rules, n, wb):
    from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
    key = (bytes(rules.to_c()), n, wb)
    if key not in _LOGICS:
        _LOGICS[key] = BatchedGameLogic(rules, n, wb)
    return _LOGICS[key]


def gpu_batch(rules, n, wb, states, G):
    lg = gpu_logic(rules, n, wb)
    b = lg.new_batch(G)
    b.upload(states)
    return b


def expand_compare_gpu(rules, n, wb, lst, tag, oracle=None):
    """Masks and counts of the positions, then every legal play of every position through do_kth_play: plays, effects and states against
    the oracle.  oracle: an Expansion of the same list computed before (oracle_expansion), else it is computed here."""
    lg = orc.GameLogic(rules, n)
    G = len(lst)
    states = pu.states_array(lst)
    b = gpu_batch(rules, n, wb, states, G)
    if oracle is None:
        oc, om = orc.batch_movegen(lg, states, G, wb)
    else:
        oc, om = oracle.counts, oracle.masks
    gc, gm = b.iter_plays()
    assert list(oc) == list(gc), tag
    assert bytes(om) == bytes(gm), tag
    cov = collections.Counter()
    if oracle is None:
        arr, ranks, total, src = pu.expand_all(states, G, oc)
    else:
        arr, ranks, total = oracle.arr, oracle.ranks, oracle.total
    if total == 0:
        return cov
    if oracle is None:
        a = pu.clone_states(arr, total)
        op, oe = orc.batch_step_kth(lg, a, total, wb, ranks)
    else:
        a, op, oe = oracle.after, oracle.plays, oracle.effects
    b2 = gpu_batch(rules, n, wb, arr, total)
    gp, ge = b2.do_kth_play(ranks)
    got = b2.download()
    same = bytes(op) == bytes(gp) and bytes(oe) == bytes(ge)
    for i in range(total):
        if not same:
            assert pu.play_tuple4(op[i]) == pu.play_tuple4(gp[i]), (tag, i)
            assert pu.effects_tuple(oe[i]) == pu.effects_tuple(ge[i]), (tag, i, pu.describe_state(arr[i], wb), pu.play_tuple4(op[i]))
        cov[(oe[i].status, oe[i].reason)] += 1
    assert pu.states_equal(a, got, total), (tag, pu.first_state_diff(a, got, total))
    b.close(); b2.close()
    return cov


# ---- comparisons shared by the host-sim and the device tests -----------------------------------------------------------------------------

def assert_same_plays_effects(tag, wb, arr, op, oe, gp, ge, total):
    for i in range(total):
        assert pu.play_tuple4(op[i]) == pu.play_tuple4(gp[i]), (tag, i, pu.describe_state(arr[i], wb))
        assert pu.effects_tuple(oe[i]) == pu.effects_tuple(ge[i]), (tag, i, pu.describe_state(arr[i], wb), pu.play_tuple4(op[i]))


def result_tuples(res, G):
    return [(res[g].value, res[g].status, res[g].reason, res[g].winner, res[g].plies) for g in range(G)]


def advanced_start(pair, label, G, seed, base, mod=None):
    """G games from start_fen(n), (7 g) % mod random plies in (the oracle's batch_random_advance): (states, plies)."""
    n, wb = pair
    rules = ruleset(pair, label)
    mod = mod or max(2, 3 * n)
    states = pu.start_states(orc, start_fen(n), rules.starting_side, wb, G)
    plies = (C.c_uint32 * G)(*[(7 * g) % mod for g in range(G)])
    orc.batch_random_advance(orc.GameLogic(rules, n), states, G, wb, seed, plies, base)
    return states, plies


# playouts: ROLLOUT_FROM_START games from the start (7 g) % (3 n) random plies in, then ROLLOUT_CRAFTED positions spread over the pair's position
# list g % 5 random plies in (random play from the start of a 14 or 15 board ends by escape, king capture or the ply cap only; the other
# terminations come from these).  Cap 300; on sides 3 .. 5 the cap at which the oracle shows finished and capped playouts side by side.
ROLLOUT_FROM_START, ROLLOUT_CRAFTED, ROLLOUT_SEED, ROLLOUT_SIM, ROLLOUT_BASE, ROLLOUT_ADVANCE_SEED = 70, 60, 5, 9, 500, 3
ROLLOUT_G = ROLLOUT_FROM_START + ROLLOUT_CRAFTED
ROLLOUT_CAP = {3: 6, 4: 8, 5: 30}


def rollout_cap(n):
    return ROLLOUT_CAP.get(n, 300)


def _slices(states, G, workers=16):
    sz, per = C.sizeof(TaflState), max(1, -(-G // workers))
    raw = bytes(states)
    return [(g0, (TaflState * min(per, G - g0)).from_buffer_copy(raw[g0 * sz:(g0 + min(per, G - g0)) * sz])) for g0 in range(0, G, per)]


Rollouts = collections.namedtuple("Rollouts", "before plies states results")


@functools.lru_cache(maxsize=None)
def rollout_expectation(pair, label):
    """before: the batch an engine starts from; plies: the random plies of its random_advance (seed ROLLOUT_ADVANCE_SEED, base ROLLOUT_BASE);
    states: what the oracle's advance gives; results: the oracle's playouts from there (on host threads: game g keeps the id base + g)."""
    from concurrent.futures import ThreadPoolExecutor
    n, wb = pair
    rules = ruleset(pair, label)
    lg, G = orc.GameLogic(rules, n), ROLLOUT_G
    lst = position_list(pair)
    crafted = [lst[(i * (len(lst) - 1)) // (ROLLOUT_CRAFTED - 1)] for i in range(ROLLOUT_CRAFTED)]
    start = pu.start_states(orc, start_fen(n), rules.starting_side, wb, ROLLOUT_FROM_START)
    before = pu.states_array([start[g] for g in range(ROLLOUT_FROM_START)] + crafted)
    plies = (C.c_uint32 * G)(*([(7 * g) % max(2, 3 * n) for g in range(ROLLOUT_FROM_START)] + [g % 5 for g in range(ROLLOUT_CRAFTED)]))
    states = pu.clone_states(before, G)
    orc.batch_random_advance(lg, states, G, wb, ROLLOUT_ADVANCE_SEED, plies, ROLLOUT_BASE)
    with ThreadPoolExecutor(max_workers=16) as ex:
        parts = list(ex.map(lambda job: result_tuples(orc.batch_rollout(lg, job[1], len(job[1]), wb, ROLLOUT_SEED, ROLLOUT_SIM, rollout_cap(n), ROLLOUT_BASE + job[0]),
                                                      len(job[1])), _slices(states, G)))
    return Rollouts(before, plies, states, [t for part in parts for t in part])


def rollout_reason_hist(pairs, labels=RULE_LABELS):
    """Counter of (status, reason) of the oracle's playouts over the pairs and rulesets."""
    return collections.Counter((t[1], t[2]) for p in pairs for label in labels for t in rollout_expectation(p, label).results)


# ---- searches ------------------------------------------------------------------------------------------------------------------------------

Search = collections.namedtuple("Search", "pair label G sims cap flags")
SEARCH_SEED, SEARCH_BASE, SEARCH_CPUCT, SEARCH_WIDTH = 2, 77, 1.0, 512
# G and sims: the oracle side of every case takes under a second on 16 host threads (15 @256: G * sims = 768 playouts of at most 64 plies;
# oracle and host-sim together 0.7 s).
# 5 @64, 4 @64, 3 @64 and the FPU_INF case on 8 @128 search longer than their widest root has children, so roots are revisited.
SEARCHES = (
    Search((15, 256), "copenhagen", 8, 96, 64, 0),              # <8, 15, PRESET_NONE> without a padding column
    Search((14, 256), "rand0", 8, 96, 64, 0),
    Search((13, 256), "copenhagen", 8, 96, 64, 0),              # the dense 13-column preset
    Search((12, 256), "copenhagen", 10, 96, 64, 0),             # no preset: streamed steps dense13, the arena stays 8 x 15
    Search((10, 128), "copenhagen", 16, 96, 96, 0),
    Search((8, 128), "brandubh", 16, 160, 96, 0),
    Search((8, 128), "copenhagen", 12, 150, 96, abi.MCTS_FLAG_FPU_INF),
    Search((6, 64), "brandubh", 24, 120, 60, 0),
    Search((5, 64), "copenhagen", 40, 200, 40, 0),
    Search((4, 64), "rand1", 40, 200, 24, 0),
    Search((3, 64), "copenhagen", 40, 60, 12, 0),
)


def search_id(s):
    return f"{pair_id(s.pair)}-{s.label}" + ("-fpu" if s.flags else "")


@functools.lru_cache(maxsize=None)
def search_expectation(s):
    """(states, {g: [(action, visits, q hex)]}, legal counts) of a case: games from the start some random plies in, the oracle's root children."""
    n, wb = s.pair
    lg = orc.GameLogic(ruleset(s.pair, s.label), n)
    if n == 3:
        # the side to move of the 3 x 3 start has no legal play (a search from such a root is not defined: the oracle books faults):
        # the first G positions of the pair's list that have one
        lst = position_list(s.pair)
        has, _ = orc.batch_movegen(lg, pu.states_array(lst), len(lst), wb, want_masks=False)
        states = pu.states_array([st for st, k in zip(lst, has) if k > 0][:s.G])
    else:
        states, _ = advanced_start(s.pair, s.label, s.G, 11, SEARCH_BASE, mod=max(2, 2 * n))
    p = abi.TaflMctsParams(s.sims, s.cap, SEARCH_CPUCT, SEARCH_SEED, 0, s.flags)
    want = pu.oracle_children_parallel(orc, lg, wb, p, [(g, states[g], SEARCH_BASE + g) for g in range(s.G)], max_children=SEARCH_WIDTH)
    counts, _ = orc.batch_movegen(lg, states, s.G, wb, want_masks=False)
    return states, want, list(counts)


def best_plays(s):
    """The first-maximum root child of every game as a TaflPlay array (all zero where the root has no visited child), from the oracle."""
    n, _wb = s.pair
    states, want, _ = search_expectation(s)
    sub = (TaflPlay * s.G)()
    for g in range(s.G):
        vs = [v for _a, v, _q in want[g]]
        if vs and max(vs) > 0 and states[g].status == abi.ONGOING:
            p = abi.action_decode(n, want[g][vs.index(max(vs))][0])
            sub[g] = TaflPlay(p.from_row, p.from_col, p.axis, p.disp)
    return sub


# ---- guided searches (the stub evaluator of tests/stub_net.py) ---------------------------------------------------------------------------------

GUIDED_PAIRS = ((15, 256), (14, 256), (4, 64))
GUIDED_SIMS, GUIDED_CPUCT, GUIDED_G = 24, 1.25, 6


def guided_edges(pair):
    """edges_per_node: above the widest root of the workload (15 x 15: the crafted position of training_rows_util has 328 legal plays)."""
    return 384 if pair[0] >= 14 else 64


@functools.lru_cache(maxsize=None)
def guided_workload(pair):
    """GUIDED_G games from the start some plies in; at 15 @256 the wide crafted position of the training-row tests in lane 0."""
    n, wb = pair
    states, _ = advanced_start(pair, "copenhagen", GUIDED_G, 13, 0, mod=max(2, 2 * n))
    if n == 15:
        from tests.training_rows_util import wide_fen
        wide = pu.start_states(orc, wide_fen(), abi.ATTACKER, wb, 1)
        C.memmove(states, wide, C.sizeof(TaflState))
    counts, _ = orc.batch_movegen(orc.GameLogic(abi.rules.COPENHAGEN, n), states, GUIDED_G, wb, want_masks=False)
    return states, list(counts)


def guided_salts():
    return [(3 * g + 1) % 256 for g in range(GUIDED_G)]


@functools.lru_cache(maxsize=None)
def guided_expectation(pair):
    """GameLogic.gmcts per game with the stub network: ([(action, visits, q hex)] per game, (sims, predicts, terminal hits))."""
    from tests import gselfplay_util as gsu
    from tests.stub_net import matrix_bytes_of
    n, wb = pair
    states, _ = guided_workload(pair)
    lg, A, salts = orc.GameLogic(abi.rules.COPENHAGEN, n), abi.action_size(n), guided_salts()
    children, counts = [], [0, 0, 0]
    for g in range(GUIDED_G):
        kids, _ns, _pri, cnt = lg.gmcts(orc.GameState.from_abi(states[g], wb), GUIDED_SIMS, GUIDED_CPUCT,
                                        lambda s, g=g: gsu.stub(matrix_bytes_of(s.board_to_matrix()), int(s.side_to_play), A, salts[g]), wb)
        children.append([(a, v, float(q).hex()) for (_p, a, v, q) in kids])
        for i in range(3):
            counts[i] += cnt[i]
    return children, tuple(counts)
