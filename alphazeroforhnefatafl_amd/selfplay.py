"""Self-play episodes that leave their training examples on the device (include/taflhip.h tafl_selfplay_record and tafl_gselfplay_*,
DESIGN.md sections 12 and 13): the executeEpisode loop of alpha-zero-general - the code base the reference's src/mcts.py belongs to -
for a whole batch of games, with random playouts (play_episodes) or the caller's network (play_guided_episodes) as the evaluator."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .abi import TaflState
from .engine import Examples, GameBatch
from .mcts import MCTSArgs, apply_root_noise


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
    (include/taflhip.h tafl_root_noise), keyed by args.noiseSeed, the game id and the move number `move_base` + moves made."""
    apply_root_noise(batch, args)
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
    mixes root noise keyed by the episode's game id and move number.  Returns (episodes closed or cut per lane, TaflEpisodeStats,
    examples recorded in all, (dropped, overflowed))."""
    apply_root_noise(batch, args)
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
