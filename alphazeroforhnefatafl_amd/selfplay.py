"""Self-play episodes that leave their training examples on the device (include/taflhip.h tafl_selfplay_record and tafl_gselfplay_*,
DESIGN.md sections 12 and 13): the executeEpisode loop of alpha-zero-general - the code base the reference's src/mcts.py belongs to -
for a whole batch of games, with random playouts (play_episodes) or the caller's network (play_guided_episodes) as the evaluator."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .abi import TaflState
from .engine import Examples, GameBatch
from .mcts import MCTSArgs, apply_eval_symmetry, apply_forced_playouts, apply_playout_cap, apply_root_noise, apply_solver


class MatchResult:
    """What play_match returns.  games[a][r]: the episodes closed or cut while evaluator a played the attackers, r = attacker win, defender
    win, draw, cut.  wins_as_attacker[e] / wins_as_defender[e]: evaluator e's wins by colour; draws, cut, games: over both seats (games
    counts the cut ones too); score: evaluator 0's (wins + draws / 2) / (games - cut), None when no game was played to its end."""

    def __init__(self, games):
        self.games = [[int(x) for x in row] for row in games]
        g = self.games
        self.wins_as_attacker = (g[0][0], g[1][0])
        self.wins_as_defender = (g[1][1], g[0][1])          # evaluator e defends in the games whose attacker is 1 - e
        self.draws, self.cut = g[0][2] + g[1][2], g[0][3] + g[1][3]
        self.games_played = sum(g[0]) + sum(g[1])
        decided = self.games_played - self.cut
        self.score = (self.wins_as_attacker[0] + self.wins_as_defender[0] + 0.5 * self.draws) / decided if decided else None

    def __repr__(self):
        return (f"MatchResult(wins_as_attacker={self.wins_as_attacker}, wins_as_defender={self.wins_as_defender}, draws={self.draws}, cut={self.cut}, "
                f"games={self.games_played}, score={self.score})")


def play_match(batch: GameBatch, nets, args: MCTSArgs, lane_moves: int, *, examples: Examples | None = None, openings: GameBatch | None = None,
               episode_moves: int = 0, swap: int = 0, temp_moves: int = 0, sample_seed: int = 1, game_id_base: int = 0, id_stride: int = 0,
               edges_per_node: int = 256, device: bool = False, buffers=None, row_multiple: int = 1) -> MatchResult:
    """A match between the evaluators nets[0] and nets[1] (include/taflhip.h tafl_gmatch_*): the episodes run of
    play_guided_selfplay in which, in episode k of lane g, evaluator (game_id_base + g + k + swap) & 1 plays the attackers, and every
    search is evaluated by the network that owns the side to move at its root.  Both speak predict_batch(boards, sides, waiting) ->
    (priors, values).  Net e is called with the first m_e rows of its buffers - its waiting leaves in ascending lane order, m_e = their
    number rounded up to `row_multiple` and capped at the batch size, so that a compiled network sees few distinct shapes - and a net
    without waiting leaves is not called.  Host route: numpy arrays go in; (priors, values) are numpy float32 arrays, ctypes float
    arrays or pointers.  device=True: `buffers` = one (boards, sides, waiting, lanes) of torch tensors on the batch's device per
    evaluator (uint8 [n, side, side], uint8 [n], uint8 [n], int32 [n]); the net gets row views of the first three and returns integer
    device pointers.  The loop is leaves -> up to two networks -> step until nothing waits, then gselfplay_end.  args.dirichletEpsilon
    must be 0: a match takes no root noise."""
    if args.dirichletEpsilon:
        raise ValueError("play_match: a match takes no root noise (args.dirichletEpsilon must be 0)")
    if args.fastSims:
        raise ValueError("play_match: a match takes no playout cap (args.fastSims must be 0)")
    if args.forcedPlayoutsK:
        raise ValueError("play_match: a match takes no forced playouts (args.forcedPlayoutsK must be 0)")
    if args.solver:
        raise ValueError("play_match: a match takes no solver (args.solver must be False)")
    if args.evalSymmetry:
        raise ValueError("play_match: a match takes no eval symmetry (args.evalSymmetry must be False)")
    n = batch.n
    batch.clear_root_noise()
    batch.clear_playout_cap()
    batch.clear_forced_playouts()
    batch.clear_solver()
    batch.clear_eval_symmetry()
    batch.gmatch_begin(examples, lane_moves, args.numMCTSSims, args.cpuct, edges_per_node, game_id_base=game_id_base, sample_seed=sample_seed,
                       temp_moves=temp_moves, episode_moves=episode_moves, id_stride=id_stride, openings=openings, swap=swap)
    ptrs = None
    if device:
        ptrs = [tuple(t.data_ptr() for t in buffers[e]) + (n,) for e in range(2)]
    while True:
        if device:
            counts = batch.gmatch_leaves(ptrs)
            rows = [buffers[e][:3] for e in range(2)]
        else:
            counts, boards, sides, waiting, _lanes = batch.gmatch_leaves()
            rows = [(boards[e], sides[e], waiting[e]) for e in range(2)]
        if not (counts[0] or counts[1]):
            break
        priors, values = [None, None], [None, None]
        for e in range(2):
            if counts[e]:
                m = min(n, -(-counts[e] // row_multiple) * row_multiple)
                priors[e], values[e] = nets[e].predict_batch(*(a[:m] for a in rows[e]))
        batch.gmatch_step([_fptr(p) for p in priors], [_fptr(v) for v in values], device=device)
    batch.gselfplay_end(want_plays=False)
    return MatchResult(batch.gmatch_stats().games)


def _fptr(a):
    """A float32 numpy array as its data pointer; anything else (None, a ctypes array or pointer, an integer device pointer) as it is."""
    return a.ctypes.data_as(C.POINTER(C.c_float)) if isinstance(a, np.ndarray) else a


def _games_over(batch: GameBatch) -> int:
    """Games of the batch that are over (one download, the status bytes counted as an array)."""
    st = np.frombuffer(batch.download(), dtype=np.uint8).reshape(batch.n, C.sizeof(TaflState))
    return int(np.count_nonzero(st[:, TaflState.status.offset]))


def play_episodes(batch: GameBatch, examples: Examples, args: MCTSArgs, max_moves: int, moves_per_run: int = 8, *, sample_seed: int = 1,
                  temp_moves: int = 0, flags: int = 0):
    """Plays every game of `batch` from its current position until it is over or has made `max_moves` moves, `moves_per_run` moves per
    device run (move_base continues the numbering, so the pieces equal one long run), recording one example per game and move in
    `examples`; then writes the results z (Examples.finalize).  The first `temp_moves` moves of an episode are drawn in proportion to
    the visit counts, the rest are the most visited plays.  Returns (examples per game, their sum, games that are over)."""
    done, over = 0, _games_over(batch)
    while done < max_moves and over < batch.n:
        k = min(moves_per_run, max_moves - done)
        batch.selfplay_record(examples, k, args.numMCTSSims, args.cpuct, args.seed, args.max_rollout_plies, game_id_base=args.game_id_base,
                              sim_offset=done * args.numMCTSSims, flags=flags, sample_seed=sample_seed, temp_moves=temp_moves,
                              move_base=done, want_plays=False)
        done += k
        over = _games_over(batch)
    examples.finalize(batch)
    lens, total = examples.counts()
    return lens, total, over


def play_guided_episodes(batch: GameBatch, examples: Examples, nnet, args: MCTSArgs, max_moves: int, *, sample_seed: int = 1,
                         temp_moves: int = 0, edges_per_node: int = 256, device: bool = False, buffers=None, move_base: int = 0):
    """play_episodes with `nnet` as the evaluator (GuidedMCTS's protocol: nnet.predict_batch(boards, sides, waiting) -> (priors, values);
    with device=True `buffers` = (boards_ptr, sides_ptr, waiting_ptr) and everything is a device pointer).  One run of `max_moves` moves
    (tafl_gselfplay_*): every game searches args.numMCTSSims simulations per move at its own pace, so the host loop is leaves -> network
    -> step until nothing waits, with no read-back per move.  Ends with Examples.finalize.  Returns (examples per game, their sum,
    games that are over).  args.dirichletEpsilon > 0 mixes Dirichlet(args.dirichletAlpha) noise into every root's priors
    (include/taflhip.h tafl_root_noise), keyed by args.noiseSeed, the game id and the move number `move_base` + moves made.
    args.fastSims > 0 turns on playout cap randomization (include/taflhip.h tafl_playout_cap): a move is full - args.numMCTSSims
    simulations, noise, recorded - with probability args.fullMoveProb, otherwise args.fastSims simulations, no noise, not recorded.
    args.forcedPlayoutsK > 0 turns on forced playouts and policy target pruning in the full moves (include/taflhip.h
    tafl_forced_playouts; batch.forced_playouts_stats() counts them).  args.solver turns on exact win/loss proofs in every search
    (include/taflhip.h tafl_solver; batch.solver_stats() counts them)."""
    apply_root_noise(batch, args)
    apply_playout_cap(batch, args)
    apply_forced_playouts(batch, args)
    apply_solver(batch, args)
    apply_eval_symmetry(batch, args)
    batch.gselfplay_begin(examples, max_moves, args.numMCTSSims, args.cpuct, edges_per_node, game_id_base=args.game_id_base,
                          sample_seed=sample_seed, temp_moves=temp_moves, move_base=move_base)
    waiting = batch.gselfplay_step()
    while waiting:
        if device:
            batch.gmcts_leaves(*buffers)
            priors, values = nnet.predict_batch(*buffers)
        else:
            priors, values = nnet.predict_batch(*batch.gmcts_leaves())
        waiting = batch.gselfplay_step(priors, values, device=device)
    batch.gselfplay_end(want_plays=False)
    examples.finalize(batch)
    lens, total = examples.counts()
    return lens, total, _games_over(batch)


def play_guided_selfplay(batch: GameBatch, examples: Examples, nnet, args: MCTSArgs, lane_moves: int, *, episode_moves: int = 0, openings: GameBatch | None = None,
                         id_stride: int = 0, game_id_base: int = 0, sample_seed: int = 1, temp_moves: int = 0, edges_per_node: int = 256, device: bool = False,
                         buffers=None):
    """Guided self-play in episodes (include/taflhip.h tafl_gselfplay_begin_episodes): every lane of `batch` plays
    `lane_moves` moves in all, and a lane whose game ends (or reaches `episode_moves` moves, 0: no cap) before that has the result
    written to the game's examples and begins its next game from its opening - the state of `openings` (None: `batch`) at this call -
    in the same round, so the evaluator's batch stays full.  Episode k of lane g has the game id game_id_base + k * id_stride + g
    (id_stride 0: the batch size; a sharded caller passes the total).  The loop is leaves -> network -> step until nothing waits
    (nnet, device and buffers as in play_guided_episodes); then Examples.finalize settles the open tails.  args.dirichletEpsilon > 0
    mixes root noise keyed by the episode's game id and move number; args.fastSims > 0 turns on playout cap randomization as in
    play_guided_episodes (mcts.playout_cap_is_full tells which moves were full; batch.playout_cap_stats() counts them), and
    args.forcedPlayoutsK > 0 forced playouts with policy target pruning in the full moves, args.solver exact win/loss proofs.  Returns
    (episodes closed or cut per lane, TaflEpisodeStats, examples recorded in all, (dropped, overflowed))."""
    apply_root_noise(batch, args)
    apply_playout_cap(batch, args)
    apply_forced_playouts(batch, args)
    apply_solver(batch, args)
    apply_eval_symmetry(batch, args)
    batch.gselfplay_begin_episodes(examples, lane_moves, args.numMCTSSims, args.cpuct, edges_per_node, game_id_base=game_id_base, sample_seed=sample_seed,
                                   temp_moves=temp_moves, episode_moves=episode_moves, id_stride=id_stride, openings=openings)
    waiting = batch.gselfplay_step()
    while waiting:
        if device:
            batch.gmcts_leaves(*buffers)
            priors, values = nnet.predict_batch(*buffers)
        else:
            priors, values = nnet.predict_batch(*batch.gmcts_leaves())
        waiting = batch.gselfplay_step(priors, values, device=device)
    batch.gselfplay_end(want_plays=False)
    episodes, stats = batch.gselfplay_episode_stats()
    examples.finalize(batch)
    _lens, total = examples.counts()
    es = examples.stats()
    return episodes, stats, total, (es.dropped, es.overflowed)
