"""Batched mirror of the reference's `MCTS` class (src/mcts.py:11-136).

`MCTS(game_batch, args).getActionProb(temp)` runs `args.numMCTSSims` simulations for every game of
the batch on the GPU (select / expand / random-rollout / backup as lock-step HIP kernels) and returns the
policy vectors of src/mcts.py:40-53.  Without a network, `predict` is the random-rollout mode of SURVEY.md §8a (uniform priors over legal plays + the value of
one seeded random playout).  With `nnet`, `predict` is the caller's network evaluated for the whole batch at once
(`GuidedMCTS`, include/taflhip.h "guided MCTS"): nnet.predict_batch(boards, sides, waiting) -> (priors, values).

With `keep_tree=True` the object keeps its tables across calls as the reference's does: a second getActionProb adds numMCTSSims
simulations to the first, and `advance(actions)` plays a move and keeps the played child's subtree (include/taflhip.h
tafl_mcts_advance).  The default (False) starts every search from an empty root.
"""
from __future__ import annotations

from dataclasses import dataclass

from .engine import GameBatch, full_per_65536  # noqa: F401


@dataclass
class MCTSArgs:
    numMCTSSims: int = 64      # src/mcts.py:37
    cpuct: float = 1.0         # src/mcts.py:112
    seed: int = 0
    max_rollout_plies: int = 512
    game_id_base: int = 0
    # Dirichlet noise at the root of a guided search (include/taflhip.h tafl_root_noise); epsilon 0: off.  The rollout mode has no priors
    # and ignores them.
    dirichletAlpha: float = 0.0
    dirichletEpsilon: float = 0.0
    noiseSeed: int = 0
    # playout cap randomization of a guided self-play run (include/taflhip.h tafl_playout_cap); fastSims 0: off.  A move is searched with
    # numMCTSSims simulations and recorded with probability fullMoveProb, otherwise with fastSims simulations and not recorded.
    fastSims: int = 0
    fullMoveProb: float = 1.0
    capSeed: int = 0
    # forced playouts and policy target pruning of a guided self-play run (include/taflhip.h tafl_forced_playouts); 0: off
    forcedPlayoutsK: float = 0.0
    # exact win/loss proofs in the searches of a guided self-play run (include/taflhip.h tafl_solver)
    solver: bool = False
    # every leaf of a guided search or self-play run is evaluated under a random board symmetry (include/taflhip.h tafl_eval_symmetry),
    # drawn from (symmetrySeed, game id, position)
    evalSymmetry: bool = False
    symmetrySeed: int = 0


def apply_root_noise(batch: GameBatch, args: MCTSArgs, move_no: int = 0):
    """The batch's root-noise setting as `args` asks for it: set, or cleared when dirichletEpsilon is 0."""
    if args.dirichletEpsilon:
        batch.set_root_noise(args.dirichletAlpha, args.dirichletEpsilon, args.noiseSeed, args.game_id_base, move_no)
    else:
        batch.clear_root_noise()


def apply_playout_cap(batch: GameBatch, args: MCTSArgs):
    """The batch's playout-cap setting as `args` asks for it: set, or cleared when fastSims is 0."""
    if args.fastSims:
        batch.set_playout_cap(args.fastSims, args.fullMoveProb, args.capSeed)
    else:
        batch.clear_playout_cap()


def apply_forced_playouts(batch: GameBatch, args: MCTSArgs):
    """The batch's forced-playouts setting as `args` asks for it: set, or cleared when forcedPlayoutsK is 0."""
    if args.forcedPlayoutsK:
        batch.set_forced_playouts(args.forcedPlayoutsK)
    else:
        batch.clear_forced_playouts()


def apply_solver(batch: GameBatch, args: MCTSArgs):
    """The batch's solver setting as `args` asks for it: set, or cleared."""
    if args.solver:
        batch.set_solver()
    else:
        batch.clear_solver()


def apply_eval_symmetry(batch: GameBatch, args: MCTSArgs):
    """The batch's eval-symmetry setting as `args` asks for it: set, or cleared."""
    if args.evalSymmetry:
        batch.set_eval_symmetry(args.symmetrySeed, args.game_id_base)
    else:
        batch.clear_eval_symmetry()


_M32 = 0xFFFFFFFF


def _fmix32(h):
    h &= _M32; h ^= h >> 16; h = (h * 0x85EBCA6B) & _M32; h ^= h >> 13; h = (h * 0xC2B2AE35) & _M32; h ^= h >> 16
    return h


def playout_cap_is_full(seed: int, gid: int, move_no: int, full_per_65536: int) -> bool:
    """Whether move `move_no` of game `gid` is a full move under a playout cap with `seed` (include/taflhip.h tafl_playout_cap, the rule
    restated in Python): what a host needs to tell which plays of a capped run were searched at full strength and recorded."""
    f = _fmix32
    slo, shi, glo, ghi = seed & _M32, (seed >> 32) & _M32, gid & _M32, (gid >> 32) & _M32
    h0, h1 = f(slo ^ f(shi + 0x9E3779B9)), f(shi ^ f(slo + 0x7F4A7C15))
    lo, hi = f(f(h0 ^ glo) + ghi), f(f(h1 ^ ghi) + glo * 0x9E3779B1)                      # game_key(seed, gid)
    lo, hi = lo ^ 0x4F555443, hi ^ 0x504C4159                                            # ^ 0x504C41594F555443
    sk = f(lo ^ ((move_no * 0x9E3779B1 + 0x7F4A7C15) & _M32)) ^ f((hi + move_no * 0x85EBCA77 + 0x165667B1) & _M32)   # sim_key(.., M)
    return (f(sk) >> 16) < full_per_65536                                                # ply_rand(.., 0) >> 16


class MCTS:
    def __init__(self, batch: GameBatch, args: MCTSArgs, keep_tree: bool = False):
        self.batch = batch
        self.args = args
        self.keep_tree = keep_tree
        self._ran = False

    def search_all(self):
        """`for i in range(numMCTSSims): self.search(canonicalBoard)` (src/mcts.py:37-38) for every game."""
        a = self.args
        self.batch.mcts_run(a.numMCTSSims, a.cpuct, a.seed, a.max_rollout_plies, a.game_id_base, keep=self.keep_tree)
        self._ran = True

    def advance(self, actions=None):
        """Play actions[g] in every game (None: the most visited root child) and keep the played child's subtree (keep_tree=True)."""
        if not self.keep_tree:
            raise ValueError("MCTS.advance needs keep_tree=True")
        return self.batch.mcts_advance(actions)

    def getActionProb(self, temp: float = 1.0):
        """src/mcts.py:28-53.  Returns a flat ctypes array [n_games * action_size] of float64.
        temp == 0 puts all mass on the FIRST maximum (the reference draws among ties with np.random)."""
        self.search_all()
        return self.batch.mcts_policy(temp)

    def root_children(self, max_children: int = 256):
        if not self._ran:
            self.search_all()
        return self.batch.mcts_root_children(max_children)

    def best_play(self):
        """src/mcts.rs:216-227 best_move (max visits)."""
        if not self._ran:
            self.search_all()
        return self.batch.mcts_best_play()


class GuidedMCTS:
    """src/mcts.py:11-136 with `nnet` as the evaluator, for every game of the batch in lock step.

    `nnet.predict_batch(boards, sides, waiting)` receives the network input of the waiting leaves — the
    board_to_matrix planes uint8 [n, side, side] (game/main.rs:55-83), the side to move [n] and a waiting flag [n] — and
    returns (priors float32 [n, action_size], values float32 [n]); rows of games that are not waiting are ignored.
    With `device=True` the three inputs are integer device pointers into buffers the caller allocated
    (`buffers=(boards_ptr, sides_ptr, waiting_ptr)`) and the outputs are device pointers too: nothing crosses PCIe.
    """

    def __init__(self, batch: GameBatch, nnet, args: MCTSArgs, edges_per_node: int = 256, device: bool = False, buffers=None,
                 keep_tree: bool = False, move_no: int = 0):
        self.batch, self.nnet, self.args, self.keep_tree, self.move_no = batch, nnet, args, keep_tree, move_no
        self.edges_per_node, self.device, self.buffers = edges_per_node, device, buffers
        self.rounds = 0
        self._ran = False

    def search_all(self):
        a, b = self.args, self.batch
        apply_root_noise(b, a, self.move_no)           # (the noise of move number self.move_no: set it before each search of a game)
        apply_eval_symmetry(b, a)
        b.gmcts_begin(a.numMCTSSims, self.edges_per_node, keep=self.keep_tree)
        waiting = b.gmcts_step(None, None, a.cpuct, a.numMCTSSims)
        while waiting:
            if self.device:
                b.gmcts_leaves(*self.buffers)
                priors, values = self.nnet.predict_batch(*self.buffers)
            else:
                priors, values = self.nnet.predict_batch(*b.gmcts_leaves())
            waiting = b.gmcts_step(priors, values, a.cpuct, a.numMCTSSims, device=self.device)
            self.rounds += 1
        self._ran = True

    def getActionProb(self, temp: float = 1.0):
        """src/mcts.py:28-53 per game: flat float64 [n_games * action_size] (temp 0: first maximum)."""
        self.search_all()
        return self.batch.gmcts_policy(temp)

    def root_children(self, max_children: int = 512):
        if not self._ran:
            self.search_all()
        return self.batch.gmcts_root_children(max_children)

    def advance(self, actions=None):
        """Play actions[g] in every game (None: the most visited root child) and keep the played child's subtree (keep_tree=True)."""
        if not self.keep_tree:
            raise ValueError("GuidedMCTS.advance needs keep_tree=True")
        return self.batch.gmcts_advance(actions)
