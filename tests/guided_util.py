"""Drivers shared by the guided-MCTS parity tests: the same lock-step loop over hostsim (CPU) and the HIP kernels (GPU)."""
import ctypes as C

from alphazeroforhnefatafl_amd.abi import TaflRootChild
from tests.stub_net import stub_predict


def stub_batch(boards, sides, waiting, n, side_len, action_size, salts):
    """nnet.predict for every waiting game: (priors float32 [n * A], values float32 [n]) as ctypes arrays."""
    pri = (C.c_float * (n * action_size))()
    val = (C.c_float * n)()
    nn = side_len * side_len
    for g in range(n):
        if not waiting[g]:
            continue
        p, v = stub_predict(bytes(boards[g * nn:(g + 1) * nn]), int(sides[g]), action_size, salts[g])
        C.memmove(C.byref(pri, 4 * g * action_size), p.ctypes.data, 4 * action_size)
        val[g] = float(v)
    return pri, val


def run_device_guided(batch, n, side_len, n_sims, c_puct, salts, edges_per_node=256, max_children=600, keep=False):
    """The same loop through the C-ABI (tafl_gmcts_begin / step / leaves / root_children): (children per game, stats, rounds).
    keep: n_sims more simulations on the retained tree."""
    from alphazeroforhnefatafl_amd import abi
    A = abi.action_size(side_len)
    batch.gmcts_begin(n_sims, edges_per_node, keep)
    w = batch.gmcts_step(None, None, c_puct, n_sims)
    rounds = 0
    while w:
        boards, sides, waiting = batch.gmcts_leaves()
        assert sum(waiting) == w
        pri, val = stub_batch(boards, sides, waiting, n, side_len, A, salts)
        w = batch.gmcts_step(pri, val, c_puct, n_sims)
        rounds += 1
    kids, cnt = batch.gmcts_root_children(max_children)
    out = [[(kids[g * max_children + i].action, kids[g * max_children + i].visits, float(kids[g * max_children + i].q).hex()) for i in range(cnt[g])]
           for g in range(n)]
    return out, batch.gmcts_stats(), rounds


def run_hostsim_guided(hs, L, states, n, n_sims, c_puct, salts, edges_per_node=256, max_children=600):
    from alphazeroforhnefatafl_amd import abi
    A = abi.action_size(hs.n)
    h = L.hs_gmcts_new(*hs._h(), states, n, n_sims, edges_per_node)
    assert h
    try:
        boards, sides, waiting = (C.c_uint8 * (n * hs.n * hs.n))(), (C.c_uint8 * n)(), (C.c_uint8 * n)()
        w = L.hs_gmcts_step(h, None, None, c_puct, n_sims)
        rounds = 0
        while w:
            L.hs_gmcts_leaves(h, boards, sides, waiting)
            pri, val = stub_batch(boards, sides, waiting, n, hs.n, A, salts)
            w = L.hs_gmcts_step(h, pri, val, c_puct, n_sims)
            rounds += 1
        kids = (TaflRootChild * (n * max_children))()
        cnt = (C.c_uint32 * n)()
        L.hs_gmcts_root_children(h, kids, max_children, cnt)
        counts = (C.c_uint64 * 4)()
        L.hs_gmcts_counts(h, counts)
        return [[(kids[g * max_children + i].action, kids[g * max_children + i].visits, float(kids[g * max_children + i].q).hex()) for i in range(cnt[g])]
                for g in range(n)], list(counts), rounds
    finally:
        L.hs_gmcts_free(h)
