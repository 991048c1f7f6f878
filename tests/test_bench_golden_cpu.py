"""CPU side of the tests at the benchmark's settings (tests/test_gpu_bench_settings.py): the Brandubh fixture is what its generator
writes today (scattered blocks regenerated with the oracle), the helpers the GPU tests lean on do what they say, and the GPU file
imports and chooses its ids without a GPU."""
import ctypes as C
import importlib.util
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflMctsParams, TaflRootChild
from oracle import oracle as orc
from tests import parity_util as pu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD_PATH = os.path.join(HERE, "golden", "bench_brandubh7_S64.json")


def _generator():
    spec = importlib.util.spec_from_file_location("make_bench_brandubh_golden", os.path.join(HERE, "golden", "make_bench_brandubh_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_brandubh_fixture_is_what_the_oracle_gives_today():
    with open(GOLD_PATH) as f:
        gold = json.load(f)
    assert os.path.getsize(GOLD_PATH) < 100_000
    gen = _generator()
    assert (gold["games"], gold["sims"], gold["max_rollout_plies"], gold["seed"], gold["c_puct"], gold["game_id_base"], gold["block"]) == \
           (gen.GAMES, gen.SIMS, gen.CAP, gen.SEED, gen.CPUCT, 0, gen.BLOCK) == (65536, 64, 512, 2, 1.0, 0, 64)
    digests = gold["sha256"]
    assert len(digests) == 1024 and len(set(digests)) == 1024 and all(len(d) == 64 for d in digests)
    rules, fen, _wb = pu.CONFIGS["brandubh7"]
    lg = orc.GameLogic(rules, abi.fen_side_len(fen))
    blocks = [0, 1, 130, 511, 512, 777, 1001, 1023]                     # both ends, both sides of the middle, scattered
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        again = list(ex.map(lambda blk: gen.block_digest(lg, blk), blocks))
    assert again == [digests[blk] for blk in blocks]


def test_block_digest_reads_the_records_it_names():
    """children_block_digests over a hand-made result: the digest depends on count, action, visits and the Q bits of the entries below
    the count, and on nothing else (play bytes, entries beyond the count)."""
    import hashlib
    import struct
    n, width = 128, 4
    kids = (TaflRootChild * (n * width))()
    cnt = (C.c_uint32 * n)(*[g % 4 for g in range(n)])
    for g in range(n):
        for j in range(width):
            k = kids[g * width + j]
            k.action, k.visits, k.q = 7 * g + j, g + j + 1, (-1.0) ** g * (0.1 + j)
    rec, c = pu.children_view(kids, cnt, n, width)
    want = []
    for blk in range(2):
        h = hashlib.sha256()
        for g in range(blk * 64, blk * 64 + 64):
            h.update(struct.pack("<I", g % 4))
            for j in range(g % 4):
                h.update(struct.pack("<IId", 7 * g + j, g + j + 1, (-1.0) ** g * (0.1 + j)))
        want.append(h.hexdigest())
    assert pu.children_block_digests(rec, c) == want
    kids[3 * width + 3].visits += 1                                      # beyond the count of game 3 (3 children): ignored
    kids[5 * width].play.from_row = 9                                    # the play bytes are not part of the record
    assert pu.children_block_digests(rec, c) == want
    kids[70 * width + 1].q = -kids[70 * width + 1].q                     # game 70 has 2 children: block 1 changes, block 0 does not
    got = pu.children_block_digests(rec, c)
    assert got[0] == want[0] and got[1] != want[1]


def test_first_children_diff_and_visit_sums():
    n, width = 6, 3
    a, b = (TaflRootChild * (n * width))(), (TaflRootChild * (n * width))()
    ca, cb = (C.c_uint32 * n)(*[2] * n), (C.c_uint32 * n)(*[2] * n)
    for buf in (a, b):
        for i in range(n * width):
            buf[i].action, buf[i].visits, buf[i].q = i, 2 * i, 0.5 * i
    ra, na = pu.children_view(a, ca, n, width)
    rb, nb = pu.children_view(b, cb, n, width)
    assert pu.first_children_diff(ra, na, rb, nb) == -1
    assert pu.root_visit_sums(ra, na).tolist() == [2 * (3 * g) + 2 * (3 * g + 1) for g in range(n)]
    b[4 * width + 2].visits = 99                                         # beyond the count: no difference
    assert pu.first_children_diff(ra, na, rb, nb) == -1
    b[4 * width + 1].q = -0.0 if b[4 * width + 1].q == 0 else np.nextafter(b[4 * width + 1].q, 1e9)   # one ulp in Q
    assert pu.first_children_diff(ra, na, rb, nb) == 4
    cb[2] = 1
    assert pu.first_children_diff(ra, na, rb, nb) == 2
    assert pu.children_of(ra, na, 1) == [(3, 6, (1.5).hex()), (4, 8, (2.0).hex())]


def test_partition_rule_and_the_ids_of_the_gpu_file():
    """search_partitions restates mcts_begin's split (waves of 64 games dealt out in order); the GPU file imports without a GPU and its
    id lists hold 0, 63, 64, G - 1, both sides of every partition boundary, and enough ids."""
    assert pu.search_partitions(65536, 2) == [(0, 32768), (32768, 65536)]
    assert pu.search_partitions(8192 + 70, 2) == [(0, 4160), (4160, 8262)]           # 130 waves -> 65 + 65, the last one short
    assert pu.search_partitions(200, 3) == [(0, 128), (128, 192), (192, 200)]         # 4 waves -> 2 + 1 + 1
    assert pu.search_partitions(100, 8) == [(0, 64), (64, 100)]                       # never more partitions than waves
    assert pu.default_search_parts(65536, False) == 2 and pu.default_search_parts(8191, False) == 1 and pu.default_search_parts(65536, True) == 1
    assert pu.boundary_ids(65536, 2) == [0, 63, 64, 32767, 32768, 65535]
    from tests import test_gpu_bench_settings as tb
    need = {"mcts_S256": 3, "mcts_S1000": 3, "mcts_mixed_positions_S64": 8, "mcts_13x13_S64": 4, "mcts_brandubh7_S64": 64}
    assert set(tb.VARIANTS) == set(need)
    for name, k in need.items():
        ids = tb.variant_ids(name)
        assert len(ids) >= k and {0, 63, 64, 65535} <= set(ids), name
        if tb.BOARDS[tb.VARIANTS[name][0]][3] != 64:
            assert {32767, 32768} <= set(ids), name
    assert sum(1 for i in tb.variant_ids("mcts_mixed_positions_S64") if i % 64 >= 56) >= 8
    # the evaluator of the guided test: exact (integers and powers of two), position-dependent, with all-zero rows
    w, table, vtable = tb.guided_tables(abi.action_size(11), 11)
    assert table.dtype == np.float32 and vtable.dtype == np.float32 and table.shape == (tb.GUIDED_K, abi.action_size(11))
    assert not table[::7].any() and table[1:7].all() and (np.abs(vtable) <= 1).all()
    lg = orc.GameLogic(abi.rules.COPENHAGEN, 11)
    base = orc.GameState(abi.boards.COPENHAGEN, abi.rules.COPENHAGEN.starting_side, 128)
    hs = set()
    for gid in range(40, 64):
        s = lg.random_advance(base, 1, gid, gid)
        m = np.array(s.board_to_matrix(), dtype=np.int64).reshape(1, -1)
        hs.add(int(tb.guided_hash(m, np.array([int(s.side_to_play)], dtype=np.int64), w)[0]))
    assert len(hs) > 12


def test_bench_settings_match_bench_py():
    """The GPU file copies bench.py's constants instead of importing it: compare them with the source text."""
    import re
    from tests import test_gpu_bench_settings as tb
    src = open(os.path.join(os.path.dirname(HERE), "bench.py")).read()
    assert int(re.search(r"^GAMES_PER_GPU = (\d+)", src, re.M).group(1)) == tb.GAMES_PER_GPU
    assert int(re.search(r'"--max-plies", type=int, default=(\d+)', src).group(1)) == tb.CAP
    assert int(re.search(r'"--seed", type=int, default=(\d+)', src).group(1)) == tb.SEED
    assert float(re.search(r'"--cpuct", type=float, default=([\d.]+)', src).group(1)) == tb.CPUCT
    for key, (board, sims, mixed, _ids) in tb.VARIANTS.items():
        call = re.search(r'out\["%s"\] = mcts_variant\("(\w+)", (\d+), \d+, \d+(, mixed=True)?\)' % key, src)
        assert call and (call.group(1), int(call.group(2)), bool(call.group(3))) == (board, sims, mixed), key
    assert 'out["selfplay_continuous_S64"] = selfplay_variant(64, 8)' in src and 'out["guided_engine_only_S64"] = guided_variant(64)' in src
    p = TaflMctsParams(64, tb.CAP, tb.CPUCT, tb.SEED, 0, 0)
    assert (p.n_sims, p.max_rollout_plies, p.seed) == (64, 512, 2)
