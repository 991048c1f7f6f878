"""Guided self-play at each game's own pace (include/taflhip.h tafl_gselfplay_*) on a real MI355X:
k_gselfplay_step against the synchronous loop through the existing entry points {gmcts_begin; steps; gmcts_root_children; the pick rule
in Python; tafl_step} on a second batch with the same states, against the oracle loop for spot games, across shards, with device
pointers and a torch network, and the rules that close a run.  Every comparison is exact except the row sum of a gathered policy, whose
bound is that of DESIGN.md section 12.  `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

from alphazeroforhnefatafl_amd import abi
from alphazeroforhnefatafl_amd.abi import TaflPlay, TaflState
from oracle import oracle as orc
from tests import examples_util as eu
from tests import gselfplay_util as gsu
from tests import parity_util as pu

pytestmark = pytest.mark.gpu

CPUCT, SEED = 1.25, 5
#         G   S  moves temp_moves  start positions (game i advanced by (7 i) mod this; 0: the start position)
SHAPES = {"brandubh7": (96, 16, 6, 3, 60),       # one full wave plus half a wave; games over at the start, ending mid-run, still going
          "copenhagen11": (70, 12, 3, 1, 36),    # two workgroups, 6 live lanes in the second
          "copenhagen13": (66, 8, 2, 1, 0),      # 256-bit words, 15-column stride
          "tablut9": (40, 12, 3, 1, 0)}
_LOGICS, _SETUP, _OWN = {}, {}, {}


def gpu_logic(rules, n, wb):
    from alphazeroforhnefatafl_amd.engine import BatchedGameLogic
    key = (bytes(rules.to_c()), n, wb)
    if key not in _LOGICS:
        _LOGICS[key] = BatchedGameLogic(rules, n, wb)
    return _LOGICS[key]


def setup(cfg):
    if cfg not in _SETUP:
        G, _S, _moves, _temp, modulus = SHAPES[cfg]
        rules, fen, wb = pu.CONFIGS[cfg]
        n = abi.fen_side_len(fen)
        olg = orc.GameLogic(rules, n)
        _SETUP[cfg] = (rules, n, wb, olg, gpu_logic(rules, n, wb), gsu.start_states(orc, olg, rules, fen, wb, G, modulus), [(3 * g + 1) % 256 for g in range(G)])
    return _SETUP[cfg]


def batch_of(glg, states, first, count):
    b = glg.new_batch(count)
    b.upload((TaflState * count)(*[states[first + g] for g in range(count)]))
    return b


device_examples = gsu.device_examples


def own_pace_run(glg, states, first, G, n, S, salts, n_moves, temp_moves, base, max_children=None):
    """The run through tafl_gselfplay_* with the stub network in host buffers: (Run with its examples, overflow marks, stats)."""
    b = batch_of(glg, states, first, G)
    ex = glg.new_examples(G, n_moves, max_children or S)
    out = gsu.device_run(b, ex, n, S, CPUCT, salts[first:first + G], n_moves, SEED, temp_moves, base=base)
    ex.close(); b.close()
    return out


def whole(cfg):
    """The own-pace run of the whole batch of a shape, run once."""
    if cfg not in _OWN:
        G, S, n_moves, temp_moves, _ = SHAPES[cfg]
        _rules, n, _wb, _olg, glg, states, salts = setup(cfg)
        _OWN[cfg] = own_pace_run(glg, states, 0, G, n, S, salts, n_moves, temp_moves, 0)
    return _OWN[cfg]


def synchronous_run(glg, states, G, n, S, salts, n_moves, temp_moves):
    """The loop the run replaces, through the existing entry points only, all games in lock step."""
    A = abi.action_size(n)
    b = batch_of(glg, states, 0, G)
    out = gsu.Run(G, n_moves)
    stopped = [False] * G
    for m in range(n_moves):
        cur, enc = b.download(), bytes(b.encode_boards())
        live = [cur[g].status == abi.ONGOING and not stopped[g] for g in range(G)]
        if not any(live):
            break
        b.gmcts_begin(S)
        w = b.gmcts_step(None, None, CPUCT, S)
        while w:
            boards, sides, waiting = b.gmcts_leaves()
            pri, val = gsu.stub_rows(boards, sides, waiting, G, n, A, salts)
            w = b.gmcts_step(gsu.fptr(pri), gsu.fptr(val), CPUCT, S)
        kids, cnt = b.gmcts_root_children(512)
        plays = (TaflPlay * G)()
        for g in range(G):
            if not live[g]:
                continue
            out.sims += S
            ch = [kids[g * 512 + j] for j in range(cnt[g])]
            vs = [c.visits for c in ch]
            if not vs:
                stopped[g] = True
                continue
            j = eu.pick_rule(vs, eu.sample_word(SEED, g, m)) if m < temp_moves else vs.index(max(vs))
            board = [list(enc[(g * n + r) * n:(g * n + r + 1) * n]) for r in range(n)]
            out.examples[g].append((board, int(cur[g].side_to_play), [c.action for c in ch], vs, ch[j].action, m))
            C.memmove(C.byref(plays[g]), C.byref(ch[j].play), C.sizeof(TaflPlay))
            out.plays[m][g] = pu.play_tuple4(ch[j].play)
            out.moves[g] = m + 1
        b.do_play(plays)
    st = b.download()
    out.states = [bytes(st[g]) for g in range(G)]
    b.close()
    return out


@pytest.mark.parametrize("cfg", list(SHAPES))
def test_own_pace_run_equals_the_synchronous_loop(cfg):
    G, S, n_moves, temp_moves, _ = SHAPES[cfg]
    _rules, n, wb, olg, glg, states, salts = setup(cfg)
    got, over, stats = whole(cfg)
    want = synchronous_run(glg, states, G, n, S, salts, n_moves, temp_moves)
    if cfg == "brandubh7":
        over0, ended, going = gsu.fates(states, want)
        assert over0 and ended and going, (over0, ended, going)
    gsu.assert_same_run(got, want, got.examples, where=cfg)
    assert stats.sims == want.sims and stats.faults == 0 and stats.waiting == 0 and not any(any(o) for o in over)
    # ten spot games against the oracle loop directly
    spots = sorted({g for g in (0, 1, 63, 64, G - 1) if g < G} | set(range(5, G, max(G // 5, 1))))[:10]
    ref = gsu.oracle_run(orc, olg, states, wb, S, CPUCT, salts, n_moves, SEED, temp_moves, games=spots)
    gsu.assert_same_run(got, ref, got.examples, games=spots, where=cfg + " oracle")


def test_shards_equal_the_whole_batch():
    """The two halves of the Brandubh batch as batches of their own, with game_id_base 0 and 48."""
    G, S, n_moves, temp_moves, _ = SHAPES["brandubh7"]
    _rules, n, _wb, _olg, glg, states, salts = setup("brandubh7")
    full, _, stats = whole("brandubh7")
    sims = 0
    for first in (0, 48):
        part, _, st = own_pace_run(glg, states, first, 48, n, S, salts, n_moves, temp_moves, first)
        sims += st.sims
        for g in range(48):
            assert [row[g] for row in part.plays] == [row[first + g] for row in full.plays], (first, g)
            assert part.moves[g] == full.moves[first + g] and part.states[g] == full.states[first + g], (first, g)
            assert part.examples[g] == full.examples[first + g], (first, g)
    assert sims == stats.sims


def test_device_pointer_route_with_a_torch_network():
    """play_guided_episodes with a small torch network whose inputs and outputs stay on the device == the same network through host
    buffers; then finalize and a device gather: every row with n_children > 0 sums to 1 within n_children * 2^-25."""
    import torch
    from alphazeroforhnefatafl_amd import BatchedGameLogic, MCTSArgs, boards, play_guided_episodes, rules
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    n, side, S, n_moves = 64, 11, 12, 2
    lg = BatchedGameLogic(rules.COPENHAGEN, side)
    A = lg.action_size
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(8 * side * side, A + 1)).to(dev).eval()

    class Net:
        def forward(self, boards_t, sides_t):
            with torch.no_grad():
                x = torch.stack([boards_t.float() / 35.0, (sides_t.float() / 8.0)[:, None, None].expand(-1, side, side)], 1)
                y = net(x)
                return torch.softmax(y[:, :A], 1).contiguous(), torch.tanh(y[:, A]).contiguous()

    class DeviceNet(Net):
        def __init__(self):
            self.boards = torch.empty((n, side, side), dtype=torch.uint8, device=dev)
            self.sides = torch.empty(n, dtype=torch.uint8, device=dev)
            self.waiting = torch.empty(n, dtype=torch.uint8, device=dev)
            self.keep = None

        def predict_batch(self, *_ptrs):
            p, v = self.forward(self.boards, self.sides)
            torch.cuda.synchronize()
            self.keep = (p, v)
            return p.data_ptr(), v.data_ptr()

    class HostNet(Net):
        def predict_batch(self, boards_, sides_, waiting):
            bt = torch.frombuffer(bytearray(bytes(boards_)), dtype=torch.uint8).reshape(n, side, side).to(dev)
            st = torch.frombuffer(bytearray(bytes(sides_)), dtype=torch.uint8).to(dev)
            p, v = self.forward(bt, st)
            p, v = p.cpu().numpy(), v.cpu().numpy()
            self.keep = (p, v)
            return p.ctypes.data_as(C.POINTER(C.c_float)), v.ctypes.data_as(C.POINTER(C.c_float))

    args = MCTSArgs(numMCTSSims=S, cpuct=1.0)
    b1 = lg.new_batch(n, boards.COPENHAGEN)
    b1.random_advance(5, (C.c_uint32 * n)(*[g % 30 for g in range(n)]))
    states = b1.download()
    b2 = lg.new_batch(n)
    b2.upload(states)
    ex1, ex2 = lg.new_examples(n, n_moves, S), lg.new_examples(n, n_moves, S)
    dn = DeviceNet()
    r1 = play_guided_episodes(b1, ex1, dn, args, n_moves, sample_seed=3, temp_moves=1, device=True,
                              buffers=(dn.boards.data_ptr(), dn.sides.data_ptr(), dn.waiting.data_ptr()))
    r2 = play_guided_episodes(b2, ex2, HostNet(), args, n_moves, sample_seed=3, temp_moves=1)
    lens = list(r1[0])
    assert (lens, r1[1], r1[2]) == (list(r2[0]), r2[1], r2[2]) and r1[1] == sum(lens) > n
    p1, m1 = b1.gselfplay_end()
    p2, m2 = b2.gselfplay_end()
    assert bytes(p1) == bytes(p2) and list(m1) == list(m2) == lens
    final = b1.download()
    assert bytes(final) == bytes(b2.download())
    assert device_examples(ex1, n, side) == device_examples(ex2, n, side)
    st = b1.gmcts_stats()
    assert st.sims == S * sum(lens) and st.faults == 0        # (a game stops only when it is over or has made its moves)
    rows = np.array([j * n + g for g in range(n) for j in range(lens[g])], np.uint32)
    _boards, _sides, pi, z, fin = ex1.gather(torch.from_numpy(rows.astype(np.int32)).to(dev), device=True)
    nc = torch.from_numpy(ex1.read(rows)[0].astype(np.int64)).to(dev)
    assert bool((nc > 0).all()) and bool(((pi != 0).sum(1) == nc).all())
    assert bool(((pi.double().sum(1) - 1.0).abs() <= nc.double() * 2.0 ** -25).all())
    over = [int(final[int(e) % n].status != abi.ONGOING) for e in rows]
    assert fin.cpu().tolist() == over and all((zz != 0) == bool(o) for zz, o in zip(z.cpu().tolist(), over))


def test_what_closes_a_run():
    from alphazeroforhnefatafl_amd._lib import TaflError
    rules, n, _wb, _olg, glg, states, salts = setup("brandubh7")
    G, A = 8, abi.action_size(n)
    b = batch_of(glg, states, 0, G)
    ex = glg.new_examples(G, 2, 8)

    def open_run():
        b.gselfplay_begin(ex, 2, 8, CPUCT, sample_seed=SEED)
        assert b.gselfplay_step() == sum(states[g].status == abi.ONGOING for g in range(G))
        boards, sides, waiting = b.gmcts_leaves()
        return gsu.stub_rows(boards, sides, waiting, G, n, A, salts[:G])

    def step_fails(pri, val):
        with pytest.raises(TaflError) as ei:
            b.gselfplay_step(gsu.fptr(pri), gsu.fptr(val))
        assert ei.value.code == -1               # TAFL_ERR_INVALID_ARG

    pri, val = open_run()
    b.gselfplay_step(gsu.fptr(pri), gsu.fptr(val))           # an open run steps
    pri, val = open_run()
    b.do_play((TaflPlay * G)())         # tafl_step writes the batch states
    step_fails(pri, val)
    pri, val = open_run()
    b.gmcts_begin(8)
    step_fails(pri, val)
    pri, val = open_run()
    b.gselfplay_end()
    step_fails(pri, val)
    other = glg.new_examples(G + 1, 2, 8)
    for bad_ex, sims in ((other, 8), (ex, 65536), (ex, 0)):
        with pytest.raises(TaflError) as ei:
            b.gselfplay_begin(bad_ex, 2, sims, CPUCT)
        assert ei.value.code == -1
    with pytest.raises(TaflError) as ei:
        b.gselfplay_begin(ex, 0, 8, CPUCT)
    assert ei.value.code == -1
