"""Host-side mirror of the reference's `GameLogic` surface (game/game/logic.rs:62-880), batched.

`BatchedGameLogic(rules, side_len)` plays the role of `GameLogic::new(rules, board_length)`;
`GameBatch` holds n `GameState<T>` values (game/game/state.rs:119-146) resident in HBM.  Method names,
argument meaning and error behaviour follow the reference: per-game rule errors come back as
`PlayInvalid` codes (game/error.rs:49-70), never as exceptions; only library / HIP failures raise.
All compute runs in HIP kernels through the C-ABI (include/taflhip.h); there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import weakref

from . import abi
from ._lib import check, lib
from .abi import (TaflEffects, TaflEpisodeOpts, TaflEpisodeStats, TaflEvalSymmetry, TaflExamplesStats, TaflForcedPlayouts, TaflForcedPlayoutsStats, TaflGmctsStats, TaflMatchIo, TaflMatchOpts, TaflMatchStats, TaflRootNoise, TaflMctsParams, TaflMctsStats, TaflPlay, TaflPlayoutCap, TaflPlayoutCapStats, TaflPoolDedupResult, TaflPoolIngestResult, TaflPoolStats, TaflPoolWeightCounters, TaflPoolWeights, TaflRolloutResult, TaflRootChild, TaflSolver, TaflSolverStats,
                  TaflSelfplayOpts, TaflState)


def full_per_65536(full_prob: float) -> int:
    """tafl_playout_cap.full_per_65536 for the probability `full_prob` of a full move: round(full_prob * 65536)."""
    return int(round(full_prob * 65536))


KC_MOVEGEN, KC_STEP, KC_ROLLOUT, KC_MCTS_TREE, KC_MCTS_ROLLOUT = range(5)


class BatchedGameLogic:
    """GameLogic{rules, board_geo} bound to one GPU (tafl_ctx)."""

    def __init__(self, rules: abi.Ruleset, side_len: int, word_bits: int | None = None, device: int = 0,
                 stream: int | None = None):
        self.rules = rules
        self.side_len = side_len
        self.word_bits = word_bits or abi.word_bits_for(side_len)
        self.device = device
        self._c_rules = rules.to_c()
        self._batches = weakref.WeakSet()   # the open GameBatch objects of this context (a batch leaves the set when it is closed or collected)
        self._h = C.c_void_p()
        check(lib().tafl_ctx_create(C.byref(self._c_rules), side_len, self.word_bits, device,
                                    C.c_void_p(stream) if stream else None, C.byref(self._h)))

    def close(self):
        """Destroys the context; batches created from it that are still open are closed first (the library refuses to destroy a
        context with live batches)."""
        if self._h:
            for b in list(self._batches):
                b.close()
            self._batches.clear()
            check(lib().tafl_ctx_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def action_size(self) -> int:
        return lib().tafl_action_size(self._h)

    @property
    def mask_words(self) -> int:
        return lib().tafl_action_mask_words(self._h)

    def sync(self):
        check(lib().tafl_sync(self._h))

    def new_batch(self, n_games: int, fen: str | None = None, side_to_play: int | None = None) -> "GameBatch":
        b = GameBatch(self, n_games)
        if fen is not None:
            b.reset_fen(fen, self.rules.starting_side if side_to_play is None else side_to_play)
        return b

    def new_examples(self, n_games: int, max_moves: int, max_children: int, search_stats: bool = False, value_targets: bool = False) -> "Examples":
        """A device-resident buffer of training examples for batches of `n_games` games: room for `max_moves` examples per game with up
        to `max_children` policy entries each (max_children >= n_sims can never overflow).  Filled by GameBatch.selfplay_record.
        search_stats: guided self-play runs also keep Qsa and the prior of every stored child (Examples.read_stats, .gather_stats);
        rollout-mode recording refuses such an object.
        value_targets (needs search_stats): episode boundaries are kept too, and Examples.value_targets computes a TD(lambda) value
        target per example."""
        return Examples(self, n_games, max_moves, max_children, search_stats, value_targets)

    def new_pool(self, capacity: int, max_children: int, search_stats: bool = False, value_targets: bool = False) -> "Pool":
        """A training pool on the device: a ring of `capacity` finished examples with up to `max_children` policy entries each, filled by
        Pool.ingest from Examples objects and sampled by Pool.sample (tafl_pool_*).  search_stats: Pool.set_search_stats(True)."""
        p = Pool(self, capacity, max_children)
        if search_stats:
            p.set_search_stats(True)
        if value_targets:
            p.set_value_targets(True)
        return p

    def state_from_fen(self, fen: str, side_to_play: int | None = None) -> TaflState:
        st = TaflState()
        side = self.rules.starting_side if side_to_play is None else side_to_play
        check(lib().tafl_state_from_fen(self._h, fen.encode(), side, C.byref(st)))
        return st

    # timing of the kernel classes (HIP events on the ctx stream)
    def timing_enable(self, on: bool = True):
        check(lib().tafl_timing_enable(self._h, int(on)))

    def timing_reset(self):
        check(lib().tafl_timing_reset(self._h))

    def timing_get(self, kernel_class: int):
        ms, k = C.c_double(), C.c_uint64()
        check(lib().tafl_timing_get(self._h, kernel_class, C.byref(ms), C.byref(k)))
        return ms.value, k.value

    def timing_get_union(self, kernel_class: int):
        """(time with at least one launch of the class in flight, sum of the launch durations) in ms since the last reset."""
        u, t = C.c_double(), C.c_double()
        check(lib().tafl_timing_get_union(self._h, kernel_class, C.byref(u), C.byref(t)))
        return u.value, t.value


class GameBatch:
    """n GameState<T> values in HBM + the batched GameLogic operations over them."""

    def __init__(self, logic: BatchedGameLogic, n_games: int):
        self.logic = logic
        self.n = n_games
        self._gsp_moves = 0               # n_moves of the last gselfplay_begin (the size of gselfplay_end's plays)
        self._h = C.c_void_p()
        check(lib().tafl_batch_create(logic._h, n_games, C.byref(self._h)))
        logic._batches.add(self)

    def close(self):
        if self._h:
            lib().tafl_batch_destroy(self._h)
            self._h = C.c_void_p()
            self.logic._batches.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- state movement -------------------------------------------------------------------------
    def reset_fen(self, fen: str, side_to_play: int):
        """GameState::new(fen, side) for every game (game/game/state.rs:136-145)."""
        check(lib().tafl_batch_reset_fen(self._h, fen.encode(), side_to_play))

    def upload(self, states, first: int = 0, count: int | None = None):
        count = self.n - first if count is None else count
        check(lib().tafl_batch_upload(self._h, states, first, count))

    def download(self, first: int = 0, count: int | None = None):
        count = self.n - first if count is None else count
        out = (TaflState * count)()
        check(lib().tafl_batch_download(self._h, out, first, count))
        return out

    # -- GameLogic surface -------------------------------------------------------------------------
    def iter_plays(self, want_masks: bool = True):
        """All legal plays of the side to move, per game: (counts, dense action masks) — get_all_possible_moves
        (game/main.rs:33-43) = iter_occupied x GameLogic::iter_plays (logic.rs:850-856)."""
        counts = (C.c_uint32 * self.n)()
        masks = (C.c_uint32 * (self.n * self.logic.mask_words))() if want_masks else None
        check(lib().tafl_movegen(self._h, counts, masks))
        return counts, masks

    def validate_play(self, plays):
        """GameLogic::validate_play (logic.rs:219-222): PlayInvalid code per game (0 = Ok)."""
        codes = (C.c_uint8 * self.n)()
        check(lib().tafl_validate(self._h, plays, codes))
        return codes

    def do_play(self, plays, want_effects: bool = True):
        """GameLogic::do_play (logic.rs:827-834) for every game; invalid plays leave that game unchanged."""
        eff = (TaflEffects * self.n)() if want_effects else None
        check(lib().tafl_step(self._h, plays, eff))
        return eff

    def do_kth_play(self, ranks):
        """Game i plays its (ranks[i] mod count)-th legal play in canonical order."""
        eff = (TaflEffects * self.n)()
        plays = (TaflPlay * self.n)()
        check(lib().tafl_step_kth(self._h, ranks, plays, eff))
        return plays, eff

    def side_can_play(self, side: int):
        """GameLogic::side_can_play (logic.rs:837-846)."""
        out = (C.c_uint8 * self.n)()
        check(lib().tafl_side_can_play(self._h, side, out))
        return out

    # -- rollouts / MCTS ------------------------------------------------------------------------------
    def rollout(self, seed: int, sim: int, max_plies: int, game_id_base: int = 0):
        out = (TaflRolloutResult * self.n)()
        check(lib().tafl_rollout(self._h, seed, sim, max_plies, game_id_base, out))
        return out

    def random_advance(self, seed: int, plies, game_id_base: int = 0):
        check(lib().tafl_random_advance(self._h, seed, plies, game_id_base))

    def mcts_reserve(self, max_sims: int):
        check(lib().tafl_mcts_reserve(self._h, max_sims))

    def mcts_run(self, n_sims: int, c_puct: float, seed: int, max_rollout_plies: int, game_id_base: int = 0,
                 sim_offset: int = 0, flags: int = 0, keep: bool = False):
        """`for i in range(numMCTSSims): self.search(canonicalBoard)` of MCTS.getActionProb (src/mcts.py:37-38) for every game.
        `flags`: abi.MCTS_FLAG_* semantics bits | abi.mcts_tune(pipeline, slots) execution tuning (never changes results).
        `keep`: continue the retained tree (abi.MCTS_FLAG_KEEP_TREE): the reference's MCTS object whose tables persist across calls."""
        p = TaflMctsParams(n_sims, max_rollout_plies, c_puct, seed, sim_offset, flags | (abi.MCTS_FLAG_KEEP_TREE if keep else 0))
        check(lib().tafl_mcts_run(self._h, C.byref(p), game_id_base))

    def mcts_run_async(self, n_sims: int, c_puct: float, seed: int, max_rollout_plies: int, game_id_base: int = 0,
                       sim_offset: int = 0, flags: int = 0, after: "GameBatch | None" = None, keep: bool = False):
        """The same search, enqueued on the batch's own streams without blocking the host (tafl_mcts_run_async): the search of another batch,
        a network, or the bookkeeping of the previous move run beside it.  `after`: hold this search back until that batch's search in
        flight is half-way through (two half-size batches started this way stay half a search apart, so that the nearly empty last rounds
        of one run under the full rounds of the other).  Join with mcts_wait(); every reader of the results joins by itself."""
        p = TaflMctsParams(n_sims, max_rollout_plies, c_puct, seed, sim_offset, flags | (abi.MCTS_FLAG_KEEP_TREE if keep else 0))
        if after is None:
            check(lib().tafl_mcts_run_async(self._h, C.byref(p), game_id_base))
        else:
            check(lib().tafl_mcts_run_async_after(self._h, C.byref(p), game_id_base, after._h))

    def selfplay_run(self, n_moves: int, n_sims: int, c_puct: float, seed: int, max_rollout_plies: int, game_id_base: int = 0,
                     sim_offset: int = 0, flags: int = 0, want_plays: bool = True):
        """n_moves x (search + most visited play) per game on the device, every game at its own pace (tafl_selfplay_run): per game the same
        as `for m in range(n_moves): mcts_run(..., sim_offset=sim_offset + m * n_sims); mcts_play_best()`.  Returns the plays [m * n + g]."""
        p = TaflMctsParams(n_sims, max_rollout_plies, c_puct, seed, sim_offset, flags)
        plays = (TaflPlay * (self.n * n_moves))() if want_plays else None
        check(lib().tafl_selfplay_run(self._h, C.byref(p), n_moves, game_id_base, plays))
        return plays

    def selfplay_record(self, examples: "Examples | None", n_moves: int, n_sims: int, c_puct: float, seed: int, max_rollout_plies: int,
                        game_id_base: int = 0, sim_offset: int = 0, flags: int = 0, sample_seed: int = 0, temp_moves: int = 0,
                        move_base: int = 0, want_plays: bool = True):
        """selfplay_run that leaves one training example per game and move in `examples` (tafl_selfplay_record): the play of move
        M = move_base + m is drawn in proportion to the visit counts while M < temp_moves (keyed by sample_seed, the global game id and M),
        the most visited one afterwards, so temp_moves = 0 plays exactly what selfplay_run plays.  `examples` None: only the plays."""
        p = TaflMctsParams(n_sims, max_rollout_plies, c_puct, seed, sim_offset, flags)
        o = TaflSelfplayOpts(sample_seed, temp_moves, move_base, 0)
        plays = (TaflPlay * (self.n * n_moves))() if want_plays else None
        check(lib().tafl_selfplay_record(self._h, C.byref(p), C.byref(o), n_moves, game_id_base, examples._h if examples is not None else None, plays))
        return plays

    def mcts_wait(self):
        """Joins the search in flight; runs the rounds its slowest games still need (tafl_mcts_wait)."""
        check(lib().tafl_mcts_wait(self._h))

    def mcts_round_trace(self, cap: int = 4096):
        """(requested, run) playouts of every round of the last search (measurement; the two-kernel pipeline only)."""
        req, run, k = (C.c_uint32 * cap)(), (C.c_uint32 * cap)(), C.c_uint32()
        check(lib().tafl_mcts_round_trace(self._h, req, run, cap, C.byref(k)))
        m = min(k.value, cap)
        return list(req[:m]), list(run[:m])

    def mcts_stats(self) -> TaflMctsStats:
        st = TaflMctsStats()
        check(lib().tafl_mcts_get_stats(self._h, C.byref(st)))
        return st

    def mcts_root_children(self, max_children: int = 256):
        kids = (TaflRootChild * (self.n * max_children))()
        cnt = (C.c_uint32 * self.n)()
        check(lib().tafl_mcts_root_children(self._h, kids, max_children, cnt))
        return kids, cnt

    def mcts_root_visits(self):
        out = (C.c_uint32 * (self.n * self.logic.action_size))()
        check(lib().tafl_mcts_root_visits(self._h, out))
        return out

    def mcts_policy(self, temp: float = 1.0):
        out = (C.c_double * (self.n * self.logic.action_size))()
        check(lib().tafl_mcts_policy(self._h, temp, out))
        return out

    def encode_boards(self, out_device_ptr: int | None = None):
        """board_to_matrix (game/main.rs:55-83) for every game: uint8 [n, side_len, side_len].  With `out_device_ptr`
        (e.g. a torch uint8 tensor's data_ptr on this device) nothing crosses PCIe; otherwise returns a host ctypes array."""
        if out_device_ptr is not None:
            check(lib().tafl_encode_boards(self._h, C.c_void_p(out_device_ptr), 1))
            return None
        out = (C.c_uint8 * (self.n * self.logic.side_len * self.logic.side_len))()
        check(lib().tafl_encode_boards(self._h, C.cast(out, C.c_void_p), 0))
        return out

    def mcts_policy_device(self, temp: float = 1.0, out_device_ptr: int | None = None, tie_seed: int = 0, game_id_base: int = 0):
        """src/mcts.py:40-53 written by a kernel, any temp >= 0; float64 [n, action_size].  temp == 0: one-hot on the first maximum, or
        with tie_seed != 0 on the seeded choice among the maxima (the reference draws it with np.random.choice)."""
        if out_device_ptr is not None:
            check(lib().tafl_mcts_policy_device_ex(self._h, temp, tie_seed, game_id_base, C.c_void_p(out_device_ptr), 1))
            return None
        out = (C.c_double * (self.n * self.logic.action_size))()
        check(lib().tafl_mcts_policy_device_ex(self._h, temp, tie_seed, game_id_base, C.cast(out, C.c_void_p), 0))
        return out

    # -- guided MCTS: the caller's network is nnet.predict (src/mcts.py:85) --------------------------------------------
    def gmcts_begin(self, max_sims: int, edges_per_node: int = 256, keep: bool = False):
        """`keep`: continue the retained guided tree (abi.GMCTS_KEEP_TREE): kept nodes keep their priors and values."""
        if keep:
            check(lib().tafl_gmcts_begin_ex(self._h, max_sims, edges_per_node, abi.GMCTS_KEEP_TREE))
        else:
            check(lib().tafl_gmcts_begin(self._h, max_sims, edges_per_node))

    def gmcts_step(self, priors=None, values=None, c_puct: float = 1.0, n_sims: int = 64, device: bool = False, want_waiting: bool = True) -> int:
        """Expand the waiting leaves with (priors float32 [n, action_size], values float32 [n]) and select the next ones.
        `priors` / `values`: ctypes float arrays (host) or integer device pointers (device=True).  Returns the games now waiting."""
        w = C.c_uint32()
        pp = C.c_void_p(priors) if isinstance(priors, int) else (C.cast(priors, C.c_void_p) if priors is not None else None)
        pv = C.c_void_p(values) if isinstance(values, int) else (C.cast(values, C.c_void_p) if values is not None else None)
        check(lib().tafl_gmcts_step(self._h, pp, pv, int(device), c_puct, n_sims, C.byref(w) if want_waiting else None))
        return w.value

    def gmcts_leaves(self, boards_ptr: int | None = None, sides_ptr: int | None = None, waiting_ptr: int | None = None):
        """Network input of the waiting leaves: (boards uint8 [n, side, side], sides uint8 [n], waiting uint8 [n]); with device
        pointers nothing crosses PCIe, otherwise host ctypes arrays are returned."""
        if boards_ptr is not None:
            check(lib().tafl_gmcts_leaves(self._h, C.c_void_p(boards_ptr), C.c_void_p(sides_ptr), C.c_void_p(waiting_ptr), 1))
            return None
        n, s = self.n, self.logic.side_len
        boards, sides, waiting = (C.c_uint8 * (n * s * s))(), (C.c_uint8 * n)(), (C.c_uint8 * n)()
        check(lib().tafl_gmcts_leaves(self._h, C.cast(boards, C.c_void_p), C.cast(sides, C.c_void_p), C.cast(waiting, C.c_void_p), 0))
        return boards, sides, waiting

    def gmcts_root_children(self, max_children: int = 512):
        kids = (TaflRootChild * (self.n * max_children))()
        cnt = (C.c_uint32 * self.n)()
        check(lib().tafl_gmcts_root_children(self._h, kids, max_children, cnt))
        return kids, cnt

    def gmcts_root_visits(self, out_device_ptr: int | None = None):
        if out_device_ptr is not None:
            check(lib().tafl_gmcts_root_visits(self._h, C.c_void_p(out_device_ptr), 1))
            return None
        out = (C.c_uint32 * (self.n * self.logic.action_size))()
        check(lib().tafl_gmcts_root_visits(self._h, C.cast(out, C.c_void_p), 0))
        return out

    def gmcts_policy(self, temp: float = 1.0, out_device_ptr: int | None = None, tie_seed: int = 0, game_id_base: int = 0):
        if out_device_ptr is not None:
            check(lib().tafl_gmcts_policy_ex(self._h, temp, tie_seed, game_id_base, C.c_void_p(out_device_ptr), 1))
            return None
        out = (C.c_double * (self.n * self.logic.action_size))()
        check(lib().tafl_gmcts_policy_ex(self._h, temp, tie_seed, game_id_base, C.cast(out, C.c_void_p), 0))
        return out

    def gmcts_stats(self) -> TaflGmctsStats:
        st = TaflGmctsStats()
        check(lib().tafl_gmcts_get_stats(self._h, C.byref(st)))
        return st

    # -- guided self-play at each game's own pace (include/taflhip.h tafl_gselfplay_*) ------------------------------------
    def gselfplay_begin(self, examples: "Examples | None", n_moves: int, n_sims: int, c_puct: float = 1.0, edges_per_node: int = 256,
                        game_id_base: int = 0, sample_seed: int = 0, temp_moves: int = 0, move_base: int = 0):
        """Opens a guided self-play run (tafl_gselfplay_begin): every game, n_moves times, searches n_sims simulations with the caller's
        evaluator, chooses its play by the rule of selfplay_record, appends the example to `examples` (None: only the plays) and plays
        it, all inside gselfplay_step.  The first gselfplay_step takes no priors."""
        o = TaflSelfplayOpts(sample_seed, temp_moves, move_base, 0)
        check(lib().tafl_gselfplay_begin(self._h, n_sims, edges_per_node, c_puct, C.byref(o), n_moves, game_id_base,
                                         examples._h if examples is not None else None))
        self._gsp_moves = n_moves

    def gselfplay_begin_episodes(self, examples: "Examples | None", lane_moves: int, n_sims: int, c_puct: float = 1.0, edges_per_node: int = 256,
                                 game_id_base: int = 0, sample_seed: int = 0, temp_moves: int = 0, episode_moves: int = 0, id_stride: int = 0,
                                 openings: "GameBatch | None" = None):
        """Opens a guided self-play run in episodes (tafl_gselfplay_begin_episodes): gselfplay_begin with `lane_moves` as each lane's move
        budget over all its games.  A lane whose game ends (or has made `episode_moves` moves, 0: no cap) with budget left gets the
        result written to that game's examples, takes its opening again - the state of `openings` (None: this batch) at this call -
        under the game id game_id_base + k * id_stride + lane (id_stride 0: the batch size), and its new root waits in the same round.
        gselfplay_step, gmcts_leaves and gselfplay_end serve the run as they serve a plain one."""
        o = TaflSelfplayOpts(sample_seed, temp_moves, 0, 0)
        eo = TaflEpisodeOpts(id_stride, episode_moves, 0)
        check(lib().tafl_gselfplay_begin_episodes(self._h, n_sims, edges_per_node, c_puct, C.byref(o), lane_moves, game_id_base,
                                                  examples._h if examples is not None else None, C.byref(eo), openings._h if openings is not None else None))
        self._gsp_moves = lane_moves

    def gselfplay_episode_stats(self):
        """(episodes closed or cut per lane [n], TaflEpisodeStats: attacker_wins, defender_wins, draws, cut) of the episodes run."""
        eps, st = (C.c_uint32 * self.n)(), TaflEpisodeStats()
        check(lib().tafl_gselfplay_episode_stats(self._h, eps, C.byref(st)))
        return eps, st

    def gselfplay_step(self, priors=None, values=None, device: bool = False, want_waiting: bool = True) -> int:
        """One round of the run: gmcts_step's arguments (the run's c_puct and n_sims).  Returns the games now waiting; 0: the run is complete."""
        w = C.c_uint32()
        pp = C.c_void_p(priors) if isinstance(priors, int) else (C.cast(priors, C.c_void_p) if priors is not None else None)
        pv = C.c_void_p(values) if isinstance(values, int) else (C.cast(values, C.c_void_p) if values is not None else None)
        check(lib().tafl_gselfplay_step(self._h, pp, pv, int(device), C.byref(w) if want_waiting else None))
        return w.value

    def gselfplay_end(self, want_plays: bool = True):
        """Closes the run (tafl_gselfplay_end): (plays [m * n + g], all-zero for a move not made, or None; moves made per game [n])."""
        plays = (TaflPlay * (self.n * self._gsp_moves))() if want_plays and self._gsp_moves else None
        moves = (C.c_uint32 * self.n)()
        check(lib().tafl_gselfplay_end(self._h, plays, moves))
        return plays, moves

    # -- match play: two evaluators in an episodes run (include/taflhip.h tafl_gmatch_*) ----------------------------------------
    def gmatch_begin(self, examples: "Examples | None", lane_moves: int, n_sims: int, c_puct: float = 1.0, edges_per_node: int = 256,
                     game_id_base: int = 0, sample_seed: int = 0, temp_moves: int = 0, episode_moves: int = 0, id_stride: int = 0,
                     openings: "GameBatch | None" = None, swap: int = 0):
        """Opens a match run (tafl_gmatch_begin): gselfplay_begin_episodes with two evaluators.  In episode k of lane g evaluator
        (game_id_base + g + k + swap) & 1 plays the attackers, and every search is evaluated by the evaluator that owns the side to move
        at its root.  The loop is gmatch_leaves -> the evaluators -> gmatch_step until both counts are 0; gselfplay_end,
        gselfplay_episode_stats, gmcts_leaves and gmcts_stats serve the run as they serve an episodes run.  Refused while root noise is set."""
        o = TaflSelfplayOpts(sample_seed, temp_moves, 0, 0)
        eo = TaflEpisodeOpts(id_stride, episode_moves, 0)
        mo = TaflMatchOpts(swap, 0)
        check(lib().tafl_gmatch_begin(self._h, n_sims, edges_per_node, c_puct, C.byref(o), lane_moves, game_id_base,
                                      examples._h if examples is not None else None, C.byref(eo), openings._h if openings is not None else None, C.byref(mo)))
        self._gsp_moves = lane_moves

    def gmatch_leaves(self, buffers=None, cap: int | None = None):
        """Each evaluator's dense batch of its waiting leaves, rows in ascending lane order (tafl_gmatch_leaves).  Host route
        (buffers None): returns (counts, boards, sides, waiting, lanes), the last four pairs of numpy arrays with `cap` rows (default:
        the batch size), of which the first counts[e] of evaluator e are written (waiting: all `cap`); the arrays are reused by the next
        call.  Device route: `buffers` = one (boards_ptr, sides_ptr, waiting_ptr, lanes_ptr, cap) per evaluator (any pointer None) and
        only (count_0, count_1) comes back.  A count above its cap raises TaflError (TAFL_ERR_CAPACITY) and writes nothing."""
        io, cnt = TaflMatchIo(), (C.c_uint32 * 2)()
        if buffers is not None:
            for e in range(2):
                io.boards[e], io.sides[e], io.waiting[e], io.lanes[e], io.cap[e] = buffers[e]
            check(lib().tafl_gmatch_leaves(self._h, C.byref(io), 1, cnt))
            return cnt[0], cnt[1]
        import numpy as np
        cap = self.n if cap is None else cap
        s = self.logic.side_len
        held = getattr(self, "_gm_host", None)
        if held is None or held[0] != cap:
            held = self._gm_host = (cap, [np.zeros((cap, s, s), np.uint8) for _ in range(2)], [np.zeros(cap, np.uint8) for _ in range(2)],
                                    [np.zeros(cap, np.uint8) for _ in range(2)], [np.zeros(cap, np.uint32) for _ in range(2)])
        _cap, boards, sides, waiting, lanes = held
        for e in range(2):
            io.boards[e], io.sides[e], io.waiting[e], io.lanes[e] = (a[e].ctypes.data for a in (boards, sides, waiting, lanes))
            io.cap[e] = cap
        check(lib().tafl_gmatch_leaves(self._h, C.byref(io), 0, cnt))
        return (cnt[0], cnt[1]), boards, sides, waiting, lanes

    def gmatch_step(self, priors, values, device: bool = False):
        """One round of the match: priors[e] (float32 [count_e, action_size]) and values[e] (float32 [count_e]) in the row order of the
        preceding gmatch_leaves, as ctypes float pointers or arrays (host) or integer device pointers (device=True); None for an
        evaluator without waiting leaves.  Runs the round, the tally and the close-and-reopen."""
        def ptrs(pair):
            out = (C.c_void_p * 2)()
            for e in range(2):
                x = pair[e]
                out[e] = None if x is None else x if isinstance(x, int) else C.cast(x, C.c_void_p)
            return out
        check(lib().tafl_gmatch_step(self._h, ptrs(priors), ptrs(values), int(device)))

    def gmatch_stats(self) -> TaflMatchStats:
        """games[a][r]: the episodes the match closed or cut while evaluator a played the attackers; r = attacker win, defender win,
        draw, cut (a game that ends on the lane's last budgeted move stays open and is not counted)."""
        st = TaflMatchStats()
        check(lib().tafl_gmatch_get_stats(self._h, C.byref(st)))
        return st

    # -- Dirichlet noise at the root of a guided search (include/taflhip.h tafl_root_noise) ----------------------------------
    def set_root_noise(self, alpha: float, epsilon: float, seed: int, game_id_base: int = 0, move_no: int = 0):
        """P' = (1 - epsilon) P + epsilon Dir(alpha) at the root of every later gmcts_begin search and gselfplay run (latched at the
        begin).  `game_id_base` / `move_no` key a lock-step search; a gselfplay run uses its own game ids and move numbers."""
        cfg = TaflRootNoise(alpha, epsilon, seed, game_id_base, move_no, 0, 0)
        check(lib().tafl_gmcts_set_root_noise(self._h, C.byref(cfg)))

    def clear_root_noise(self):
        check(lib().tafl_gmcts_set_root_noise(self._h, None))

    # -- a random board symmetry per leaf evaluation (include/taflhip.h tafl_eval_symmetry) --------------------------------------
    def set_eval_symmetry(self, seed: int, game_id_base: int = 0):
        """Every leaf of every later gmcts_begin search and gselfplay run (latched at the begin) is shown to the evaluator under one of
        the eight board symmetries, drawn from (seed, game id, position), and its priors are mapped back.  `game_id_base` keys a
        lock-step search; a gselfplay run uses its own game ids.  A match refuses the setting."""
        cfg = TaflEvalSymmetry(seed, game_id_base, 0)
        check(lib().tafl_gmcts_set_eval_symmetry(self._h, C.byref(cfg)))

    def clear_eval_symmetry(self):
        check(lib().tafl_gmcts_set_eval_symmetry(self._h, None))

    def gmcts_leaf_symmetry(self, out_device_ptr: int | None = None):
        """The symmetry (0 .. 7) each waiting leaf is shown under, uint8 [n]; 0 for a game that does not wait and with the setting off
        (tafl_gmcts_leaf_symmetry)."""
        if out_device_ptr is not None:
            check(lib().tafl_gmcts_leaf_symmetry(self._h, C.c_void_p(out_device_ptr), 1))
            return None
        out = (C.c_uint8 * self.n)()
        check(lib().tafl_gmcts_leaf_symmetry(self._h, C.cast(out, C.c_void_p), 0))
        return out

    # -- playout cap randomization of a guided self-play run (include/taflhip.h tafl_playout_cap) ------------------------------
    def set_playout_cap(self, fast_sims: int, full_prob: float, seed: int = 0):
        """Every later gselfplay_begin / gselfplay_begin_episodes run (latched at the begin) searches a move at full strength - n_sims
        simulations, root noise if set, the example recorded - with probability round(full_prob * 65536) / 65536 and otherwise with
        `fast_sims` simulations, no noise and no example; the class is a function of (seed, game id, move number)."""
        cfg = TaflPlayoutCap(seed, fast_sims, full_per_65536(full_prob), 0)
        check(lib().tafl_gselfplay_set_playout_cap(self._h, C.byref(cfg)))

    def clear_playout_cap(self):
        check(lib().tafl_gselfplay_set_playout_cap(self._h, None))

    def playout_cap_stats(self) -> TaflPlayoutCapStats:
        """The moves the capped run that is open, or was last, made per class (tafl_gselfplay_playout_cap_stats)."""
        st = TaflPlayoutCapStats()
        check(lib().tafl_gselfplay_playout_cap_stats(self._h, C.byref(st)))
        return st

    # -- forced playouts and policy target pruning of a guided self-play run (include/taflhip.h tafl_forced_playouts) -----------
    def set_forced_playouts(self, k: float):
        """Every later gselfplay_begin / gselfplay_begin_episodes run (latched at the begin) forces, in the search of a full move, each
        visited root child to at least sqrt(k * p * Ns) visits and prunes the visits the search did not confirm from what it draws the
        play from and records."""
        cfg = TaflForcedPlayouts(k, 0)
        check(lib().tafl_gselfplay_set_forced_playouts(self._h, C.byref(cfg)))

    def clear_forced_playouts(self):
        check(lib().tafl_gselfplay_set_forced_playouts(self._h, None))

    def forced_playouts_stats(self) -> TaflForcedPlayoutsStats:
        """Forced simulations, pruned visits, pruned children and full moves of the run that is open, or was last
        (tafl_gselfplay_forced_playouts_stats)."""
        st = TaflForcedPlayoutsStats()
        check(lib().tafl_gselfplay_forced_playouts_stats(self._h, C.byref(st)))
        return st

    # -- exact win/loss proofs in the searches of a guided self-play run (include/taflhip.h tafl_solver) ---------------------------
    def set_solver(self):
        """Every later gselfplay_begin / gselfplay_begin_episodes run (latched at the begin) back-propagates win/loss proofs beside the
        values: its searches skip moves that lose, end once the root is decided, and keep proven losses out of the play and the example."""
        cfg = TaflSolver(0)
        check(lib().tafl_gselfplay_set_solver(self._h, C.byref(cfg)))

    def clear_solver(self):
        check(lib().tafl_gselfplay_set_solver(self._h, None))

    def solver_stats(self) -> TaflSolverStats:
        """Proven roots and nodes, skipped simulations, pruned visits and children and the moves of the run that is open, or was last
        (tafl_gselfplay_solver_stats)."""
        st = TaflSolverStats()
        check(lib().tafl_gselfplay_solver_stats(self._h, C.byref(st)))
        return st

    def root_noise_eval(self, alpha: float, epsilon: float, seed: int, game_id_base: int = 0, move_no: int = 0, out_device_ptr: int | None = None):
        """eta of tafl_root_noise_eval for every game's current state: float64 [n * action_size], zero off the legal actions."""
        cfg = TaflRootNoise(alpha, epsilon, seed, game_id_base, move_no, 0, 0)
        if out_device_ptr is not None:
            check(lib().tafl_root_noise_eval(self._h, C.byref(cfg), C.c_void_p(out_device_ptr), 1))
            return None
        out = (C.c_double * (self.n * self.logic.action_size))()
        check(lib().tafl_root_noise_eval(self._h, C.byref(cfg), C.cast(out, C.c_void_p), 0))
        return out

    def gmcts_root_priors(self, out_device_ptr: int | None = None):
        """Dense Ps[root] of the guided search, float64 [n * action_size] (all zero for a root that is not expanded)."""
        if out_device_ptr is not None:
            check(lib().tafl_gmcts_root_priors(self._h, C.c_void_p(out_device_ptr), 1))
            return None
        out = (C.c_double * (self.n * self.logic.action_size))()
        check(lib().tafl_gmcts_root_priors(self._h, C.cast(out, C.c_void_p), 0))
        return out

    def mcts_play_best(self, want_results: bool = True):
        """Every game plays the most visited root play of its last search, on the device (tafl_mcts_play_best)."""
        if not want_results:
            check(lib().tafl_mcts_play_best(self._h, None, None))
            return None
        plays, eff = (TaflPlay * self.n)(), (TaflEffects * self.n)()
        check(lib().tafl_mcts_play_best(self._h, plays, eff))
        return plays, eff

    def mcts_best_play(self):
        plays = (TaflPlay * self.n)()
        visits = (C.c_uint32 * self.n)()
        check(lib().tafl_mcts_best_play(self._h, plays, visits))
        return plays, visits

    # -- subtree reuse (include/taflhip.h tafl_mcts_advance) ------------------------------------------------------------
    def _advance(self, fn, actions, want_results: bool):
        acts = None
        if actions is not None:
            actions = list(actions)
            if len(actions) != self.n:
                raise ValueError(f"advance: {len(actions)} actions for {self.n} games (use abi.ACTION_NONE to leave a game alone)")
            acts = (C.c_uint32 * self.n)(*[int(a) & 0xFFFFFFFF for a in actions])
        if not want_results:
            check(fn(self._h, acts, None, None))
            return None
        plays, eff = (TaflPlay * self.n)(), (TaflEffects * self.n)()
        check(fn(self._h, acts, plays, eff))
        return plays, eff

    def mcts_advance(self, actions=None, want_results: bool = True):
        """Play actions[g] (dense action index; abi.ACTION_NONE leaves the game alone; None: the most visited root child) and make that
        child the root of the retained tree (tafl_mcts_advance).  Returns (plays, effects) unless want_results is False."""
        return self._advance(lib().tafl_mcts_advance, actions, want_results)

    def gmcts_advance(self, actions=None, want_results: bool = True):
        """tafl_gmcts_advance: mcts_advance on the guided tree."""
        return self._advance(lib().tafl_gmcts_advance, actions, want_results)

    def mcts_tree_nodes(self):
        """Nodes per game in the retained rollout-mode tree (0: none)."""
        out = (C.c_uint32 * self.n)()
        check(lib().tafl_mcts_tree_nodes(self._h, out))
        return out

    def gmcts_tree_nodes(self):
        """Nodes per game in the retained guided tree (0: none)."""
        out = (C.c_uint32 * self.n)()
        check(lib().tafl_gmcts_tree_nodes(self._h, out))
        return out


class Examples:
    """Training examples (board, side to move, sparse search policy, play, result z) in HBM (tafl_examples).  Example j of game g has the
    index j * n_games + g.  The object outlives runs and batches: an episode may be recorded in several runs, a trainer may keep several."""

    def __init__(self, logic: BatchedGameLogic, n_games: int, max_moves: int, max_children: int, search_stats: bool = False, value_targets: bool = False):
        self.logic = logic
        self.n_games, self.max_moves, self.max_children = n_games, max_moves, max_children
        self.search_stats, self.has_value_targets = bool(search_stats), bool(value_targets)
        self._h = C.c_void_p()
        flags = (abi.EXAMPLES_SEARCH_STATS if search_stats else 0) | (abi.EXAMPLES_VALUE_TARGETS if value_targets else 0)
        check(lib().tafl_examples_create_ex(logic._h, n_games, max_moves, max_children, flags, C.byref(self._h)))
        logic._batches.add(self)          # closed with the context, like its batches

    def close(self):
        if self._h:
            lib().tafl_examples_destroy(self._h)
            self._h = C.c_void_p()
            self.logic._batches.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        """Every game back to 0 examples, the counters back to 0."""
        check(lib().tafl_examples_clear(self._h))

    def counts(self):
        """(examples per game [n_games], their sum)."""
        out, tot = (C.c_uint32 * self.n_games)(), C.c_uint64()
        check(lib().tafl_examples_counts(self._h, out, C.byref(tot)))
        return out, tot.value

    def stats(self) -> TaflExamplesStats:
        """dropped (a game already held max_moves), overflowed (more than max_children visited root children), bad_index, device_bytes."""
        st = TaflExamplesStats()
        check(lib().tafl_examples_get_stats(self._h, C.byref(st)))
        return st

    def finalize(self, batch: GameBatch):
        """z and the final mark of every example from the CURRENT status of its game in `batch`: +1 / -1 / 1e-4 seen from the example's
        side to move; examples of games still going on keep z = 0, final = 0 (call it again after the next run)."""
        check(lib().tafl_examples_finalize(self._h, batch._h))

    def read(self, index):
        """The sparse form of the examples `index` as numpy arrays: (n_children [k], overflow [k], played [k], move_no [k],
        actions [k, max_children], visits [k, max_children]) - the visited root children in canonical order (tafl_examples_read)."""
        import numpy as np
        idx = np.ascontiguousarray(index, dtype=np.uint32)
        k, K = int(idx.size), self.max_children
        nc, ov, pl, mv = np.zeros(k, np.uint32), np.zeros(k, np.uint8), np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        acts, vis = np.zeros((k, K), np.uint32), np.zeros((k, K), np.uint32)
        vp = C.c_void_p
        check(lib().tafl_examples_read(self._h, idx.ctypes.data_as(vp), k, nc.ctypes.data_as(vp), ov.ctypes.data_as(vp), pl.ctypes.data_as(vp),
                                       mv.ctypes.data_as(vp), acts.ctypes.data_as(vp), vis.ctypes.data_as(vp)))
        return nc, ov, pl, mv, acts, vis

    def read_stats(self, index):
        """(q [k, max_children], prior [k, max_children]) float32 of the stored children of the examples `index`, in the order of
        read()'s actions: Qsa and the root prior as the search held them (tafl_examples_read_stats; needs search_stats)."""
        import numpy as np
        idx = np.ascontiguousarray(index, dtype=np.uint32)
        k, K = int(idx.size), self.max_children
        q, pr = np.zeros((k, K), np.float32), np.zeros((k, K), np.float32)
        vp = C.c_void_p
        check(lib().tafl_examples_read_stats(self._h, idx.ctypes.data_as(vp), k, q.ctypes.data_as(vp), pr.ctypes.data_as(vp)))
        return q, pr

    def gather_stats(self, index, device: bool = False):
        """(value [k], surprise [k]) float32 of the examples `index`: the visit-weighted mean of the stored children's Qsa and
        KL(search policy || prior) in nats (tafl_examples_gather_stats; needs search_stats).  device as in gather()."""
        vp = C.c_void_p
        if device:
            import torch
            idx = index.contiguous()
            if idx.dtype != torch.int32 or not idx.is_cuda or idx.device.index != self.logic.device:
                raise ValueError("gather_stats(device=True): index must be an int32 tensor on the context's device")
            k = int(idx.numel())
            value, surprise = torch.empty((k,), dtype=torch.float32, device=idx.device), torch.empty((k,), dtype=torch.float32, device=idx.device)
            torch.cuda.current_stream(idx.device).synchronize()          # the library writes on its own stream
            check(lib().tafl_examples_gather_stats(self._h, vp(idx.data_ptr()), k, vp(value.data_ptr()), vp(surprise.data_ptr()), 1))
            self.logic.sync()
            return value, surprise
        import numpy as np
        idx = np.ascontiguousarray(index, dtype=np.uint32)
        k = int(idx.size)
        value, surprise = np.zeros(k, np.float32), np.zeros(k, np.float32)
        check(lib().tafl_examples_gather_stats(self._h, idx.ctypes.data_as(vp), k, value.ctypes.data_as(vp), surprise.ctypes.data_as(vp), 0))
        return value, surprise

    def value_targets(self, lam: float, settle_unfinished: bool = False) -> abi.TaflValueTargetsResult:
        """A TD(lambda) value target per example from the search values of the positions that follow it in its episode, ending in the
        result of a finished game or, for a cut or open episode, in its last search value (tafl_examples_value_targets; needs
        value_targets).  settle_unfinished: the rows of unfinished episodes also get that last value as z and final = 2, so that
        Pool.ingest takes them.  Returns episodes_closed, episodes_unfinished, rows_with_target, rows_settled.  The result stands
        until clear(), finalize() or the next run that records into the object."""
        cfg, out = abi.TaflValueTargetsCfg(lam=lam, flags=abi.VT_SETTLE_UNFINISHED if settle_unfinished else 0), abi.TaflValueTargetsResult()
        check(lib().tafl_examples_value_targets(self._h, C.byref(cfg), C.byref(out)))
        return out

    def gather_targets(self, index, device: bool = False):
        """(target float32 [k], kind uint8 [k], ep_end uint8 [k]) of the examples `index`: the value target, 0 / 1 / 2 for no target /
        from a closed episode / from an unfinished one, and 1 for the last example of an episode (tafl_examples_gather_targets).
        device as in gather()."""
        vp = C.c_void_p
        if device:
            import torch
            idx = index.contiguous()
            if idx.dtype != torch.int32 or not idx.is_cuda or idx.device.index != self.logic.device:
                raise ValueError("gather_targets(device=True): index must be an int32 tensor on the context's device")
            k = int(idx.numel())
            target = torch.empty((k,), dtype=torch.float32, device=idx.device)
            kind, ep_end = torch.empty((k,), dtype=torch.uint8, device=idx.device), torch.empty((k,), dtype=torch.uint8, device=idx.device)
            torch.cuda.current_stream(idx.device).synchronize()          # the library writes on its own stream
            check(lib().tafl_examples_gather_targets(self._h, vp(idx.data_ptr()), k, vp(target.data_ptr()), vp(kind.data_ptr()), vp(ep_end.data_ptr()), 1))
            self.logic.sync()
            return target, kind, ep_end
        import numpy as np
        idx = np.ascontiguousarray(index, dtype=np.uint32)
        k = int(idx.size)
        target, kind, ep_end = np.zeros(k, np.float32), np.zeros(k, np.uint8), np.zeros(k, np.uint8)
        check(lib().tafl_examples_gather_targets(self._h, idx.ctypes.data_as(vp), k, target.ctypes.data_as(vp), kind.ctypes.data_as(vp), ep_end.ctypes.data_as(vp), 0))
        return target, kind, ep_end

    def gather(self, index, sym=None, device: bool = False):
        """Minibatch rows (boards uint8 [k, n, n], sides uint8 [k], pi float32 [k, action_size], z float32 [k], final uint8 [k]) of the
        examples `index` under the board symmetries `sym` (0..7 each, None: identity).  device=False: `index` / `sym` are sequences or
        numpy arrays and numpy arrays come back.  device=True: they are torch tensors (int32 / uint8) on the context's device, torch
        tensors on that device come back and nothing crosses PCIe."""
        n, A = self.logic.side_len, self.logic.action_size
        if device:
            import torch
            dev = index.device
            k = int(index.numel())
            idx = index.contiguous()
            if idx.dtype != torch.int32 or not idx.is_cuda or idx.device.index != self.logic.device:
                raise ValueError("gather(device=True): index must be an int32 tensor on the context's device")
            sy = None
            if sym is not None:
                sy = sym.contiguous()
                if sy.dtype != torch.uint8 or sy.device != dev or sy.numel() != k:
                    raise ValueError("gather(device=True): sym must be a uint8 tensor on the same device, one per index")
            boards = torch.empty((k, n, n), dtype=torch.uint8, device=dev)
            sides = torch.empty((k,), dtype=torch.uint8, device=dev)
            pi = torch.empty((k, A), dtype=torch.float32, device=dev)
            z = torch.empty((k,), dtype=torch.float32, device=dev)
            fin = torch.empty((k,), dtype=torch.uint8, device=dev)
            torch.cuda.current_stream(dev).synchronize()          # the library writes on its own stream
            check(lib().tafl_examples_gather(self._h, C.c_void_p(idx.data_ptr()), C.c_void_p(sy.data_ptr()) if sy is not None else None, k,
                                             C.c_void_p(boards.data_ptr()), C.c_void_p(sides.data_ptr()), C.c_void_p(pi.data_ptr()),
                                             C.c_void_p(z.data_ptr()), C.c_void_p(fin.data_ptr()), 1))
            self.logic.sync()
            return boards, sides, pi, z, fin
        import numpy as np
        idx = np.ascontiguousarray(index, dtype=np.uint32)
        k = int(idx.size)
        sy = None if sym is None else np.ascontiguousarray(sym, dtype=np.uint8)
        if sy is not None and sy.size != k:
            raise ValueError("gather: one sym per index")
        boards, sides = np.zeros((k, n, n), np.uint8), np.zeros((k,), np.uint8)
        pi, z, fin = np.zeros((k, A), np.float32), np.zeros((k,), np.float32), np.zeros((k,), np.uint8)
        check(lib().tafl_examples_gather(self._h, idx.ctypes.data_as(C.c_void_p), sy.ctypes.data_as(C.c_void_p) if sy is not None else None, k,
                                         boards.ctypes.data_as(C.c_void_p), sides.ctypes.data_as(C.c_void_p), pi.ctypes.data_as(C.c_void_p),
                                         z.ctypes.data_as(C.c_void_p), fin.ctypes.data_as(C.c_void_p), 0))
        return boards, sides, pi, z, fin


class Pool:
    """A fixed-capacity window over finished training examples in HBM (tafl_pool).  The q-th row ever taken lives in slot q % capacity;
    the live rows are the newest min(written, capacity), minus what trim removed.  It outlives the Examples objects it was filled from."""

    def __init__(self, logic: BatchedGameLogic, capacity: int, max_children: int):
        self.logic = logic
        self.capacity, self.max_children = capacity, max_children
        self._h = C.c_void_p()
        check(lib().tafl_pool_create(logic._h, capacity, max_children, C.byref(self._h)))
        logic._batches.add(self)          # closed with the context, like its batches

    def close(self):
        if self._h:
            lib().tafl_pool_destroy(self._h)
            self._h = C.c_void_p()
            self.logic._batches.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def ingest(self, examples: Examples):
        """Takes every finished example of `examples` (final = 1, with a policy) in ascending index order as one generation; the object
        is not modified (clear it afterwards).  Returns (taken, skipped_open, skipped_overflow) of this call."""
        out = TaflPoolIngestResult()
        check(lib().tafl_pool_ingest(self._h, examples._h, C.byref(out)))
        return out.taken, out.skipped_open, out.skipped_overflow

    def trim(self, keep_generations: int):
        """Only the rows of the newest `keep_generations` ingests stay live (numItersForTrainExamplesHistory)."""
        check(lib().tafl_pool_trim(self._h, keep_generations))

    def clear(self):
        """Empties the pool and zeroes its counters."""
        check(lib().tafl_pool_clear(self._h))

    def stats(self) -> TaflPoolStats:
        """written, live, ingests, oldest_generation, skipped_open, skipped_overflow, bad_slot, device_bytes."""
        st = TaflPoolStats()
        check(lib().tafl_pool_get_stats(self._h, C.byref(st)))
        return st

    def _outputs(self, k, device, dev=None):
        n, A = self.logic.side_len, self.logic.action_size
        if device:
            import torch
            return (torch.empty((k, n, n), dtype=torch.uint8, device=dev), torch.empty((k,), dtype=torch.uint8, device=dev),
                    torch.empty((k, A), dtype=torch.float32, device=dev), torch.empty((k,), dtype=torch.float32, device=dev))
        import numpy as np
        return np.zeros((k, n, n), np.uint8), np.zeros((k,), np.uint8), np.zeros((k, A), np.float32), np.zeros((k,), np.float32)

    def sample(self, count: int, seed: int, step: int, row_base: int = 0, symmetries: bool = True, device: bool = False):
        """`count` uniformly drawn live rows (with replacement) as (boards uint8 [count, n, n], sides uint8, pi float32 [count, action_size],
        z float32, slot, sym): row i is drawn from (seed, step, row_base + i) alone, so rank k of a data-parallel trainer passes
        row_base = k * count.  symmetries: one of the eight board symmetries per row, else the identity.  device=True: torch tensors on
        the context's device come back (slot int32, sym uint8) and nothing crosses PCIe; otherwise numpy arrays (slot uint32)."""
        flags = abi.POOL_SAMPLE_SYM if symmetries else 0
        vp = C.c_void_p
        if device:
            import torch
            dev = torch.device("cuda", self.logic.device)
            out = self._outputs(count, True, dev)
            slot, sym = torch.empty((count,), dtype=torch.int32, device=dev), torch.empty((count,), dtype=torch.uint8, device=dev)
            torch.cuda.current_stream(dev).synchronize()          # the library writes on its own stream
            check(lib().tafl_pool_sample(self._h, seed, step, row_base, count, flags, *[vp(t.data_ptr()) for t in out], vp(slot.data_ptr()), vp(sym.data_ptr()), 1))
            self.logic.sync()
            return (*out, slot, sym)
        import numpy as np
        out = self._outputs(count, False)
        slot, sym = np.zeros((count,), np.uint32), np.zeros((count,), np.uint8)
        check(lib().tafl_pool_sample(self._h, seed, step, row_base, count, flags, *[a.ctypes.data_as(vp) for a in out], slot.ctypes.data_as(vp), sym.ctypes.data_as(vp), 0))
        return (*out, slot, sym)

    def gather(self, slots, sym=None, device: bool = False):
        """(boards, sides, pi, z) of the rows in `slots` under the board symmetries `sym` (0..7 each, None: identity): the bytes
        Examples.gather gave for the source examples.  device=False: sequences or numpy arrays in, numpy arrays out; a slot that is not
        live raises.  device=True: torch tensors (int32 / uint8) on the context's device in and out; a slot that is not live gives an
        all-zero row and counts in stats().bad_slot."""
        vp = C.c_void_p
        if device:
            import torch
            sl = slots.contiguous()
            if sl.dtype != torch.int32 or not sl.is_cuda or sl.device.index != self.logic.device:
                raise ValueError("gather(device=True): slots must be an int32 tensor on the context's device")
            k = int(sl.numel())
            sy = None
            if sym is not None:
                sy = sym.contiguous()
                if sy.dtype != torch.uint8 or sy.device != sl.device or sy.numel() != k:
                    raise ValueError("gather(device=True): sym must be a uint8 tensor on the same device, one per slot")
            out = self._outputs(k, True, sl.device)
            torch.cuda.current_stream(sl.device).synchronize()          # the library writes on its own stream
            check(lib().tafl_pool_gather(self._h, vp(sl.data_ptr()), vp(sy.data_ptr()) if sy is not None else None, k, *[vp(t.data_ptr()) for t in out], 1))
            self.logic.sync()
            return out
        import numpy as np
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        k = int(sl.size)
        sy = None if sym is None else np.ascontiguousarray(sym, dtype=np.uint8)
        if sy is not None and sy.size != k:
            raise ValueError("gather: one sym per slot")
        out = self._outputs(k, False)
        check(lib().tafl_pool_gather(self._h, sl.ctypes.data_as(vp), sy.ctypes.data_as(vp) if sy is not None else None, k, *[a.ctypes.data_as(vp) for a in out], 0))
        return out

    # ---- weighted sampling (tafl_pool_set_weighting / _set_weights / _get_weights / _sample_weighted / _weight_stats) ----
    def set_weighting(self, ingest_weight):
        """Switches weighted sampling on: one uint32 weight per slot, `ingest_weight` for every slot now (if it was off) and for every row
        a later ingest stores.  None switches it off and frees its buffers (the default: the pool behaves and allocates as without it)."""
        if ingest_weight is None:
            check(lib().tafl_pool_set_weighting(self._h, None))
            return
        w = TaflPoolWeights(ingest_weight=ingest_weight)
        check(lib().tafl_pool_set_weighting(self._h, C.byref(w)))

    def _device_u32(self, t, what, k=None):
        import torch
        t = t.contiguous()
        if t.dtype != torch.int32 or not t.is_cuda or t.device.index != self.logic.device or (k is not None and t.numel() != k):
            raise ValueError(f"{what} must be an int32 tensor on the context's device" + ("" if k is None else ", one per slot"))
        return t

    def set_weights(self, slots, weights, device: bool = False):
        """Every live slot named holds the maximum of the weights given for it afterwards (duplicates in any order); 0 silences a row.
        device=False: sequences or numpy arrays; a slot that is not live raises before anything is written.  device=True: int32 torch
        tensors on the context's device (the bits of a uint32); such an entry is skipped and counts in weight_stats().bad_slot."""
        vp = C.c_void_p
        if device:
            import torch
            sl = self._device_u32(slots, "set_weights(device=True): slots")
            wt = self._device_u32(weights, "set_weights(device=True): weights", int(sl.numel()))
            torch.cuda.current_stream(sl.device).synchronize()          # the library works on its own stream
            check(lib().tafl_pool_set_weights(self._h, vp(sl.data_ptr()), vp(wt.data_ptr()), int(sl.numel()), 1))
            self.logic.sync()
            return
        import numpy as np
        sl, wt = np.ascontiguousarray(slots, dtype=np.uint32), np.ascontiguousarray(weights, dtype=np.uint32)
        if sl.size != wt.size:
            raise ValueError("set_weights: one weight per slot")
        check(lib().tafl_pool_set_weights(self._h, sl.ctypes.data_as(vp), wt.ctypes.data_as(vp), int(sl.size), 0))

    def weights(self, slots):
        """The weights of `slots`: a numpy uint32 array for a sequence or numpy array (a slot that is not live raises), an int32 tensor for an
        int32 tensor on the context's device (0 for a slot that is not live)."""
        vp = C.c_void_p
        if hasattr(slots, "data_ptr"):
            import torch
            sl = self._device_u32(slots, "weights: a slot tensor")
            out = torch.empty_like(sl)
            torch.cuda.current_stream(sl.device).synchronize()
            check(lib().tafl_pool_get_weights(self._h, vp(sl.data_ptr()), int(sl.numel()), vp(out.data_ptr()), 1))
            self.logic.sync()
            return out
        import numpy as np
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        out = np.zeros(sl.size, np.uint32)
        check(lib().tafl_pool_get_weights(self._h, sl.ctypes.data_as(vp), int(sl.size), out.ctypes.data_as(vp), 0))
        return out

    def sample_weighted(self, count: int, seed: int, step: int, row_base: int = 0, symmetries: bool = True, device: bool = False):
        """`count` live rows drawn with replacement in proportion to their weights, as (boards, sides, pi, z, slot, sym, weight, total) in the
        shapes of `sample`: weight[i] is the weight of the row drawn, total (an int) the sum over the live rows, so weight / total is
        the probability the row was drawn with.  Row i depends on (seed, step, row_base + i), the live window and the weights alone."""
        flags = abi.POOL_SAMPLE_SYM if symmetries else 0
        vp = C.c_void_p
        if device:
            import torch
            dev = torch.device("cuda", self.logic.device)
            out = self._outputs(count, True, dev)
            slot, sym = torch.empty((count,), dtype=torch.int32, device=dev), torch.empty((count,), dtype=torch.uint8, device=dev)
            weight, total = torch.empty((count,), dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int64, device=dev)
            torch.cuda.current_stream(dev).synchronize()          # the library writes on its own stream
            check(lib().tafl_pool_sample_weighted(self._h, seed, step, row_base, count, flags, *[vp(t.data_ptr()) for t in out], vp(slot.data_ptr()), vp(sym.data_ptr()),
                                                  vp(weight.data_ptr()), vp(total.data_ptr()), 1))
            self.logic.sync()
            return (*out, slot, sym, weight, int(total.item()) & 0xFFFFFFFFFFFFFFFF)
        import numpy as np
        out = self._outputs(count, False)
        slot, sym, weight = np.zeros((count,), np.uint32), np.zeros((count,), np.uint8), np.zeros((count,), np.uint32)
        total = C.c_uint64(0)
        check(lib().tafl_pool_sample_weighted(self._h, seed, step, row_base, count, flags, *[a.ctypes.data_as(vp) for a in out], slot.ctypes.data_as(vp), sym.ctypes.data_as(vp),
                                              weight.ctypes.data_as(vp), C.cast(C.byref(total), vp), 0))
        return (*out, slot, sym, weight, int(total.value))

    # ---- search statistics per row (tafl_pool_set_search_stats / _gather_stats / _weights_from_surprise) ----
    def set_search_stats(self, on: bool = True):
        """The pool carries the search value and the policy surprise of every row it ingests (only from Examples created with
        search_stats).  Allowed while the pool holds no live row; clear() keeps the setting."""
        check(lib().tafl_pool_set_search_stats(self._h, int(bool(on))))

    def gather_stats(self, slots, device: bool = False):
        """(value [k], surprise [k]) float32 of the rows in `slots`.  device=False: a slot that is not live raises.  device=True: int32
        tensor in, tensors out; a slot that is not live gives zeros and counts in stats().bad_slot."""
        vp = C.c_void_p
        if device:
            import torch
            sl = self._device_u32(slots, "gather_stats(device=True): slots")
            k = int(sl.numel())
            value, surprise = torch.empty((k,), dtype=torch.float32, device=sl.device), torch.empty((k,), dtype=torch.float32, device=sl.device)
            torch.cuda.current_stream(sl.device).synchronize()          # the library writes on its own stream
            check(lib().tafl_pool_gather_stats(self._h, vp(sl.data_ptr()), k, vp(value.data_ptr()), vp(surprise.data_ptr()), 1))
            self.logic.sync()
            return value, surprise
        import numpy as np
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        k = int(sl.size)
        value, surprise = np.zeros(k, np.float32), np.zeros(k, np.float32)
        check(lib().tafl_pool_gather_stats(self._h, sl.ctypes.data_as(vp), k, value.ctypes.data_as(vp), surprise.ctypes.data_as(vp), 0))
        return value, surprise

    # ---- value targets per row (tafl_pool_set_value_targets / _gather_targets) ----
    def set_value_targets(self, on: bool = True):
        """The pool carries the value target and its kind of every row it ingests (only from Examples created with value_targets whose
        value_targets() result stands).  Needs search statistics on; allowed while the pool holds no live row; clear() keeps the setting."""
        check(lib().tafl_pool_set_value_targets(self._h, int(bool(on))))

    def gather_targets(self, slots, device: bool = False):
        """(target float32 [k], kind uint8 [k]) of the rows in `slots`, with the rules of gather_stats for slots that are not live."""
        vp = C.c_void_p
        if device:
            import torch
            sl = self._device_u32(slots, "gather_targets(device=True): slots")
            k = int(sl.numel())
            target, kind = torch.empty((k,), dtype=torch.float32, device=sl.device), torch.empty((k,), dtype=torch.uint8, device=sl.device)
            torch.cuda.current_stream(sl.device).synchronize()          # the library writes on its own stream
            check(lib().tafl_pool_gather_targets(self._h, vp(sl.data_ptr()), k, vp(target.data_ptr()), vp(kind.data_ptr()), 1))
            self.logic.sync()
            return target, kind
        import numpy as np
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        k = int(sl.size)
        target, kind = np.zeros(k, np.float32), np.zeros(k, np.uint8)
        check(lib().tafl_pool_gather_targets(self._h, sl.ctypes.data_as(vp), k, target.ctypes.data_as(vp), kind.ctypes.data_as(vp), 0))
        return target, kind

    def weights_from_surprise(self, base: int, per_nat: float, generation: int = 0):
        """Every live row of ingest `generation` (0: every live row) gets the weight min(2^32 - 1, base + floor(surprise * per_nat)): an
        assignment on the device, nothing is read back.  Needs weighting and search statistics on."""
        cfg = abi.TaflPoolSurpriseWeights(base=base, generation=generation, per_nat=per_nat)
        check(lib().tafl_pool_weights_from_surprise(self._h, C.byref(cfg)))
        self.logic.sync()

    # ---- de-duplication of positions (tafl_pool_dedup / _gather_dedup / _weights_from_dedup) ----
    def dedup(self, symmetries: bool = False, key_bits: int = 64) -> TaflPoolDedupResult:
        """Groups the live rows by position (side to move and board; symmetries: images under the eight board symmetries are one
        position) and keeps, per live slot, the slot of the group's newest row, the group's size and its mean result.  Returns live,
        distinct, largest, collisions, device_bytes.  The result stands until the next ingest, trim or clear.  key_bits below 64 makes
        keys collide on purpose (tests, measuring collisions)."""
        cfg = abi.TaflPoolDedupCfg(flags=abi.POOL_DEDUP_SYMMETRIES if symmetries else 0, key_bits=key_bits)
        out = TaflPoolDedupResult()
        check(lib().tafl_pool_dedup(self._h, C.byref(cfg), C.byref(out)))
        return out

    def free_dedup(self):
        """Frees everything dedup allocated and drops its result."""
        check(lib().tafl_pool_dedup(self._h, None, None))

    def gather_dedup(self, slots, device: bool = False):
        """(rep uint32 [k], mult uint32 [k], zmean float32 [k]) of the rows in `slots`.  device=False: a slot that is not live raises.
        device=True: int32 tensor in, tensors out (rep and mult int32); a slot that is not live gives zeros and counts in stats().bad_slot."""
        vp = C.c_void_p
        if device:
            import torch
            sl = self._device_u32(slots, "gather_dedup(device=True): slots")
            k = int(sl.numel())
            rep, mult = torch.empty((k,), dtype=torch.int32, device=sl.device), torch.empty((k,), dtype=torch.int32, device=sl.device)
            zmean = torch.empty((k,), dtype=torch.float32, device=sl.device)
            torch.cuda.current_stream(sl.device).synchronize()          # the library writes on its own stream
            check(lib().tafl_pool_gather_dedup(self._h, vp(sl.data_ptr()), k, vp(rep.data_ptr()), vp(mult.data_ptr()), vp(zmean.data_ptr()), 1))
            self.logic.sync()
            return rep, mult, zmean
        import numpy as np
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        k = int(sl.size)
        rep, mult, zmean = np.zeros(k, np.uint32), np.zeros(k, np.uint32), np.zeros(k, np.float32)
        check(lib().tafl_pool_gather_dedup(self._h, sl.ctypes.data_as(vp), k, rep.ctypes.data_as(vp), mult.ctypes.data_as(vp), zmean.ctypes.data_as(vp), 0))
        return rep, mult, zmean

    def weights_from_dedup(self, scale: int, divide: bool = False, representatives: bool = False):
        """Every live row gets max(1, scale // mult) - every distinct position is then drawn equally often; divide: the weight it has
        is divided by mult instead (0 stays 0, at least 1 otherwise); representatives: `scale` for the newest row of every group and 0
        for the others.  An assignment on the device, nothing is read back.  Needs weighting on and a dedup result that stands."""
        flags = (abi.POOL_DEDUP_DIVIDE if divide else 0) | (abi.POOL_DEDUP_REPRESENTATIVES if representatives else 0)
        cfg = abi.TaflPoolDedupWeights(scale=scale, flags=flags)
        check(lib().tafl_pool_weights_from_dedup(self._h, C.byref(cfg)))
        self.logic.sync()

    def weight_stats(self) -> TaflPoolWeightCounters:
        """enabled, ingest_weight, total_weight, positive, bad_slot, rebuilds, device_bytes (all zero while weighting is off)."""
        st = TaflPoolWeightCounters()
        check(lib().tafl_pool_weight_stats(self._h, C.byref(st)))
        return st

    def read(self, slots):
        """The sparse form of the rows in `slots` as numpy arrays: (n_children [k], move_no [k], generation [k], actions [k, max_children],
        visits [k, max_children]) (tafl_pool_read; not a hot path)."""
        import numpy as np
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        k, K = int(sl.size), self.max_children
        nc, mv, gen = np.zeros(k, np.uint32), np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        acts, vis = np.zeros((k, K), np.uint32), np.zeros((k, K), np.uint32)
        vp = C.c_void_p
        check(lib().tafl_pool_read(self._h, sl.ctypes.data_as(vp), k, nc.ctypes.data_as(vp), mv.ctypes.data_as(vp), gen.ctypes.data_as(vp),
                                   acts.ctypes.data_as(vp), vis.ctypes.data_as(vp)))
        return nc, mv, gen, acts, vis
