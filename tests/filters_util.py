"""Inputs of the pre-filter tests (tests/test_hostsim_filters.py on the host, tests/test_gpu_filters.py on the device): four rulesets and,
for each, the crafted rare-rule positions of tests/rare_workloads.py, kings ringed by attackers but for one tile that an attacker can
reach, kings on every edge, by every corner and by the throne between flanking defenders, and the start position.  No GPU, no library."""
import functools
import random

from alphazeroforhnefatafl_amd import abi
from oracle import oracle as orc
from tests import parity_util as pu
from tests import rare_workloads as rw

Config = rw.Config
CONFIGS = {c.name: c for c in (
    Config("copenhagen11", abi.rules.COPENHAGEN, 11, 128, False),
    Config("brandubh7", abi.rules.BRANDUBH, 7, 64, False),
    Config("tablut9", abi.rules.TABLUT, 9, 128, False),
    Config("weak_armed11", abi.rules.COPENHAGEN.replace(king_strength=abi.WEAK), 11, 128, False),
)}
START = {"copenhagen11": abi.boards.COPENHAGEN, "brandubh7": abi.boards.BRANDUBH, "tablut9": abi.boards.TABLUT, "weak_armed11": abi.boards.COPENHAGEN}


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------

def _corners(n):
    return {(0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1)}


def king_capture_positions(rng, n, wb, count, by_throne):
    """The king (anywhere; beside or on the throne with probability by_throne) with attackers on his neighbours but one, and an attacker
    that can slide onto it."""
    out, t = [], n // 2
    while len(out) < count:
        b = pu._blank(n, wb)
        k = rng.choice([(t - 1, t), (t + 1, t), (t, t - 1), (t, t + 1), (t, t)]) if rng.random() < by_throne else (rng.randrange(n), rng.randrange(n))
        if k in _corners(n):
            continue
        special = _corners(n) | {(t, t)}
        nbs = [(k[0] + dr, k[1] + dc) for dr, dc in ((1, 0), (-1, 0), (0, 1), (0, -1)) if 0 <= k[0] + dr < n and 0 <= k[1] + dc < n]
        gap = rng.choice(nbs)
        if gap in special:
            continue
        b["king"] = k
        b["att"] = {nb for nb in nbs if nb != gap and nb not in special and rng.random() < 0.85}
        lines = []
        for dr, dc in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            r, c = gap[0] + dr, gap[1] + dc
            while 0 <= r < n and 0 <= c < n and (r, c) != k and (r, c) not in b["att"] and (r, c) not in special:
                lines.append((r, c))
                r, c = r + dr, c + dc
        if not lines:
            continue
        b["att"].add(rng.choice(lines))
        taken = set(nbs) | {k} | set(lines) | special
        for _ in range(rng.randrange(2, 9)):
            tile = (rng.randrange(n), rng.randrange(n))
            if tile not in taken and tile not in b["att"] and tile not in b["def"]:
                (b["def"] if rng.random() < 0.6 else b["att"]).add(tile)
        out.append(pu._to_state(b, abi.ATTACKER))
    return out


def edge_king_spots(n):
    """(row, col): the middle of each edge, both neighbours of every corner, the four neighbours of the throne."""
    m, t, L = n // 2, n // 2, n - 1
    return [(0, m), (L, m), (m, 0), (m, L), (0, 1), (1, 0), (0, L - 1), (1, L), (L, 1), (L - 1, 0), (L, L - 1), (L - 1, L),
            (t - 1, t), (t + 1, t), (t, t - 1), (t, t + 1)]


def edge_king_positions(rng, n, wb, per_spot):
    """The king on every spot of edge_king_spots; on an edge, between two defenders of his line at random distances, with the two lines
    behind the edge sparsely filled by either side - fort candidates that the inner-line tests must sort."""
    out, L = [], n - 1
    for spot in edge_king_spots(n):
        for _ in range(per_spot):
            b = pu._blank(n, wb)
            b["king"] = spot
            r, c = spot
            if r in (0, L) or c in (0, L):
                along_row = r in (0, L)
                pos = c if along_row else r
                at = (lambda p, d: (abs(r - d), p)) if along_row else (lambda p, d: (p, abs(c - d)))       # tile at line position p, depth d
                lo, hi = (rng.randrange(0, pos) if pos > 0 else None), (rng.randrange(pos + 1, n) if pos < L else None)
                for p in (lo, hi):
                    if p is not None and rng.random() < 0.9:
                        b["def"].add(at(p, 0))
                for p in range(n):
                    for d in (1, 2):
                        x = rng.random()
                        if x < 0.12:
                            b["att"].add(at(p, d))
                        elif x < 0.45:
                            b["def"].add(at(p, d))
            for _ in range(rng.randrange(3, 10)):
                tile = (rng.randrange(n), rng.randrange(n))
                if tile != spot and tile not in b["def"] and tile not in b["att"] and tile not in _corners(n) | {(n // 2, n // 2)}:
                    (b["def"] if rng.random() < 0.4 else b["att"]).add(tile)
            b["def"].discard(spot)
            b["att"].discard(spot)
            b["att"] -= _corners(n)
            b["def"] -= _corners(n) | b["att"]
            out.append(pu._to_state(b, abi.DEFENDER if rng.random() < 0.7 else abi.ATTACKER))
    return out


@functools.lru_cache(maxsize=None)
def workload(name):
    """(states, G, plies per game, {kind: (first, end)})"""
    cfg = CONFIGS[name]
    rng = random.Random(61)
    kinds = [(k, s, 12) for k, s in rw._crafted(rng, cfg, 96, True)]
    sbt = cfg.rules.king_strength == abi.STRONG_BY_THRONE
    kinds.append(("king", king_capture_positions(rng, cfg.n, cfg.wb, 4000 if sbt else 3000, 0.9 if sbt else 0.2), 3))
    if cfg.rules.exit_fort:
        kinds.append(("more forts", pu.exit_fort_positions(rng, cfg.n, cfg.wb, 400), 6))
    kinds.append(("more enclosures", pu.enclosure_positions(rng, cfg.n, cfg.wb, 300), 6))
    kinds.append(("edge king", edge_king_positions(rng, cfg.n, cfg.wb, 24), 6))
    start = pu.start_states(orc, START[name], cfg.rules.starting_side, cfg.wb, 64)
    kinds.append(("start", [start[i] for i in range(64)], 160))
    lst, plies, spans = [], [], {}
    for kind, states, n_plies in kinds:
        spans[kind] = (len(lst), len(lst) + len(states))
        lst += states
        plies += [n_plies] * len(states)
    return pu.states_array(lst), len(lst), plies, spans
