/*
 * taflhip.h — C-ABI of the MI355X-native batched Hnefatafl engine (libtaflhip.so).
 *
 * This is the drop-in boundary for ONE hot path of payelmuk91/AlphaZeroForHnefatafl:
 * batched move generation + env step + random rollout + MCTS over many concurrent games.
 * The reference has no FFI; the surface a host uses there is the `GameLogic` method set over
 * `GameState<T>` values (game/game/logic.rs:62-880, game/game/state.rs:119-146) and, for search,
 * `MCTS.getActionProb` (src/mcts.py:28-53).  Every entry point below cites the reference
 * interface it replaces.  Plain C: opaque handles, POD structs, pointers + sizes; no C++ or
 * torch types.  All functions return 0 on success and a negative `tafl_status` on failure
 * (message via tafl_last_error()).  Per-game rule errors are returned as per-game codes, never
 * as a failed call (reference: `Result<_, PlayInvalid>`, game/error.rs:49-70).
 *
 * There is NO CPU fallback in the library: every compute entry point runs HIP kernels on a
 * gfx950 device and fails with TAFL_ERR_NO_DEVICE when none is usable.
 */
#ifndef TAFLHIP_H
#define TAFLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TAFLHIP_ABI_VERSION 1

/* ---- vocabulary (numeric values mirror the reference enums) ------------------------------ */

/* Side — game/pieces.rs:13-16 (`Attacker = 0, Defender = 8`). */
#define TAFL_ATTACKER 0
#define TAFL_DEFENDER 8

/* PieceType one-hot — game/pieces.rs:31-38.  Only King/Soldier exist on a bitfield board. */
#define TAFL_PT_KING      0x01
#define TAFL_PT_SOLDIER   0x02
#define TAFL_PT_KNIGHT    0x04
#define TAFL_PT_COMMANDER 0x08
#define TAFL_PT_GUARD     0x10
#define TAFL_PT_MERCENARY 0x20

/* PieceSet(u16) — game/pieces.rs:157-273: bit = piece_type << side (attackers low byte,
 * defenders high byte). */
typedef uint16_t tafl_pieceset;
#define TAFL_PS_NONE 0x0000u
#define TAFL_PS_ALL  0xFFFFu
#define TAFL_PS_TYPE(pt) ((tafl_pieceset)((pt) | ((pt) << 8)))   /* PieceSet::from_piece_type */
#define TAFL_PS_PIECE(pt, side) ((tafl_pieceset)((pt) << (side))) /* PieceSet::from_piece */
#define TAFL_PS_SIDE(side) ((tafl_pieceset)(0xFFu << (side)))     /* PieceSet::from(Side) */

/* Axis — game/tiles.rs:167-170 (`Vertical = 0, Horizontal = 0x80`). */
#define TAFL_AXIS_VERTICAL   0x00
#define TAFL_AXIS_HORIZONTAL 0x80

/* ThroneRule — game/rules.rs:5-17 (declaration order). */
enum { TAFL_THRONE_NOTHRONE = 0, TAFL_THRONE_NOPASS = 1, TAFL_THRONE_KINGPASS = 2,
       TAFL_THRONE_NOENTRY = 3, TAFL_THRONE_KINGENTRY = 4 };
/* KingStrength — game/rules.rs:21-30. */
enum { TAFL_KING_STRONG = 0, TAFL_KING_STRONG_BY_THRONE = 1, TAFL_KING_WEAK = 2 };
/* KingAttack — game/rules.rs:33-42. */
enum { TAFL_KING_ARMED = 0, TAFL_KING_ANVIL = 1, TAFL_KING_HAMMER = 2 };
/* EnclosureWinRules — game/rules.rs:64-70; 0 = `None`. */
enum { TAFL_ENCL_NONE = 0, TAFL_ENCL_WITH_EDGE_ACCESS = 1, TAFL_ENCL_WITHOUT_EDGE_ACCESS = 2 };

/* PlayInvalid — game/error.rs:49-70, declaration order, shifted by one so that 0 = valid. */
enum { TAFL_PLAY_OK = 0, TAFL_PLAY_WRONG_PLAYER = 1, TAFL_PLAY_NO_PIECE = 2,
       TAFL_PLAY_OUT_OF_BOUNDS = 3, TAFL_PLAY_NO_COMMON_AXIS = 4, TAFL_PLAY_BLOCKED_BY_PIECE = 5,
       TAFL_PLAY_MOVE_THROUGH_BLOCKED_TILE = 6, TAFL_PLAY_MOVE_ONTO_BLOCKED_TILE = 7,
       TAFL_PLAY_TOO_FAR = 8, TAFL_PLAY_GAME_OVER = 9 };

/* GameStatus / GameOutcome — game/game/mod.rs:16-70. */
enum { TAFL_STATUS_ONGOING = 0, TAFL_STATUS_WIN = 1, TAFL_STATUS_DRAW = 2 };
/* WinReason — game/game/mod.rs:17-33 (declaration order). */
enum { TAFL_WIN_KING_ESCAPED = 0, TAFL_WIN_EXIT_FORT = 1, TAFL_WIN_KING_CAPTURED = 2,
       TAFL_WIN_ALL_CAPTURED = 3, TAFL_WIN_ENCLOSED = 4, TAFL_WIN_NO_PLAYS = 5,
       TAFL_WIN_REPETITION = 6 };
/* DrawReason — game/game/mod.rs:36-42. */
enum { TAFL_DRAW_REPETITION = 0, TAFL_DRAW_NO_PLAYS = 1 };
/* Build-defined rollout terminations (the reference has no rollout). */
enum { TAFL_ROLLOUT_REASON_PLY_CAP = 14, TAFL_ROLLOUT_REASON_STUCK = 15 };

/* library status codes */
typedef enum {
    TAFL_OK = 0,
    TAFL_ERR_INVALID_ARG = -1,
    TAFL_ERR_NO_DEVICE = -2,
    TAFL_ERR_HIP = -3,
    TAFL_ERR_PARSE = -4,
    TAFL_ERR_UNSUPPORTED = -5,
    TAFL_ERR_OOM = -6,
    TAFL_ERR_CAPACITY = -7
} tafl_status;

/* ---- POD structs --------------------------------------------------------------------------- */

/* Ruleset — game/rules.rs:83-117, field for field (Option<..> flattened with a has_ flag). */
typedef struct tafl_rules {
    uint8_t  edge_escape;             /* bool                                   rules.rs:86  */
    uint8_t  king_strength;           /* TAFL_KING_STRONG...                    rules.rs:89  */
    uint8_t  king_attack;             /* TAFL_KING_ARMED...                     rules.rs:91  */
    uint8_t  has_shieldwall;          /* Option<ShieldwallRules>::is_some       rules.rs:93  */
    uint8_t  sw_corners_may_close;    /* ShieldwallRules.corners_may_close      rules.rs:56  */
    uint8_t  exit_fort;               /* bool                                   rules.rs:95  */
    uint8_t  throne_movement;         /* TAFL_THRONE_...                        rules.rs:97  */
    uint8_t  starting_side;           /* TAFL_ATTACKER / TAFL_DEFENDER          rules.rs:105 */
    uint8_t  enclosure_win;           /* TAFL_ENCL_... (0 = None)               rules.rs:107 */
    uint8_t  has_repetition_rule;     /* Option<RepetitionRule>::is_some        rules.rs:109 */
    uint8_t  rep_is_loss;             /* RepetitionRule.is_loss                 rules.rs:79  */
    uint8_t  draw_on_no_plays;        /* bool                                   rules.rs:112 */
    uint8_t  linnaean_capture;        /* bool                                   rules.rs:116 */
    uint8_t  _pad0[3];
    tafl_pieceset sw_captures;        /* ShieldwallRules.captures               rules.rs:58  */
    tafl_pieceset may_enter_corners;  /*                                        rules.rs:99  */
    tafl_pieceset hostility_throne;   /* HostilityRules.throne                  rules.rs:47  */
    tafl_pieceset hostility_corners;  /* HostilityRules.corners                 rules.rs:48  */
    tafl_pieceset hostility_edge;     /* HostilityRules.edge                    rules.rs:49  */
    tafl_pieceset slow_pieces;        /*                                        rules.rs:103 */
    uint32_t n_repetitions;           /* RepetitionRule.n_repetitions           rules.rs:76  */
} tafl_rules;                         /* 32 bytes */

/* Play — game/play.rs:22-27 (`from: Tile{row,col}`, `movement: AxisOffset{axis,displacement}`,
 * game/tiles.rs:11-17,108-111). 4 bytes. */
typedef struct tafl_play {
    uint8_t from_row;
    uint8_t from_col;
    uint8_t axis;        /* TAFL_AXIS_VERTICAL (0) or TAFL_AXIS_HORIZONTAL (0x80) */
    int8_t  disp;        /* signed displacement along the axis */
} tafl_play;

/* GameState<T> — game/game/state.rs:119-132 with BitfieldBoardState<T> (game/board/state.rs:116-121)
 * flattened.  `att`/`def` are the reference integers as little-endian 64-bit limbs, SAME bit
 * positions: tile bit = row*ROW_WIDTH + col (game/bitfield.rs:72-74; ROW_WIDTH 7/11/15 for
 * 64/128/256-bit words, :178-180) and the king's (row, col) in the top nibble of the most
 * significant byte of `def` / `att` (game/board/state.rs:127-147) — a Rust host can transmute a
 * u64/u128/U256.  Only the first word_bits/64 limbs are used. */
#define TAFL_MAX_LIMBS 4
typedef struct tafl_state {
    uint64_t att[TAFL_MAX_LIMBS];
    uint64_t def[TAFL_MAX_LIMBS];
    uint32_t turn;                 /* GameState.turn                       state.rs:131 */
    uint32_t plays_since_capture;  /* GameState.plays_since_capture        state.rs:127 */
    uint32_t rep_ring[4];          /* RepetitionTracker.recent_plays, OLDEST FIRST (state.rs:46,
                                      utils.rs:30-81); 0 = None, else TAFL_REP_PACK(...) */
    uint16_t attacker_reps;        /* state.rs:42 */
    uint16_t defender_reps;        /* state.rs:43 */
    uint8_t  attacker_mid_pair;    /* state.rs:44 */
    uint8_t  defender_mid_pair;    /* state.rs:45 */
    uint8_t  side_to_play;         /* TAFL_ATTACKER / TAFL_DEFENDER        state.rs:123 */
    uint8_t  status;               /* TAFL_STATUS_*                        state.rs:129 */
    uint8_t  reason;               /* WinReason / DrawReason when over */
    uint8_t  winner;               /* Side when status == WIN */
    uint8_t  side_len;             /* BitfieldBoardState.side_len          board/state.rs:120 */
    uint8_t  _pad;
} tafl_state;                      /* 104 bytes */

/* ShortPlayRecord (game/game/state.rs:15-19) packed into 32 bits, bit 31 = Some. */
#define TAFL_REP_PACK(side, from_row, from_col, axis, disp, captured)                        \
    (0x80000000u | ((uint32_t)((side) ? 1u : 0u) << 30) | ((uint32_t)((captured) ? 1u : 0u) << 29) | \
     ((uint32_t)((axis) ? 1u : 0u) << 28) | ((uint32_t)((from_row) & 0xFF) << 16) |                  \
     ((uint32_t)((from_col) & 0xFF) << 8) | ((uint32_t)((uint8_t)(disp))))

/* PlayEffects — game/game/mod.rs:56-61 — as a capture mask in board-word layout plus the
 * outcome; `code` is the PlayInvalid code when the play was rejected (state left unchanged). */
typedef struct tafl_effects {
    uint64_t captures[TAFL_MAX_LIMBS]; /* bit row*ROW_WIDTH+col set for each captured tile */
    uint8_t  code;                     /* TAFL_PLAY_* (0 = executed) */
    uint8_t  status;                   /* TAFL_STATUS_* after the play */
    uint8_t  reason;
    uint8_t  winner;
    uint8_t  n_captures;
    uint8_t  _pad[3];
} tafl_effects;                        /* 40 bytes */

/* Random-rollout result (build-defined; see DESIGN.md "Rollout policy"). */
typedef struct tafl_rollout_result {
    int8_t   value;     /* +1 / -1 / 0 from the perspective of the side to move at the start */
    uint8_t  status;    /* TAFL_STATUS_* at the end (ONGOING when capped/stuck) */
    uint8_t  reason;    /* WinReason/DrawReason or TAFL_ROLLOUT_REASON_* */
    uint8_t  winner;
    uint32_t plies;     /* plies played */
} tafl_rollout_result;  /* 8 bytes */

/* One root child after MCTS: the visited edges (s_root, a) of src/mcts.py:41 (`Nsa`), :128-133 (`Qsa`). */
typedef struct tafl_root_child {
    tafl_play play;
    uint32_t  action;   /* dense action index, see tafl_action_size() */
    uint32_t  visits;   /* Nsa */
    double    q;        /* Qsa */
} tafl_root_child;      /* 24 bytes */

typedef struct tafl_mcts_params {
    uint32_t n_sims;           /* args.numMCTSSims   src/mcts.py:37  */
    uint32_t max_rollout_plies;
    double   c_puct;           /* args.cpuct         src/mcts.py:112 */
    uint64_t seed;
    uint32_t sim_offset;       /* salt of the playouts' RNG key (normally 0): predict(s) of the random-rollout search is ONE playout from s with
                                  simulation word sim_offset + leaf key(s) - "leaf key" = MurmurHash3_x86_32, seeded with the side length, over
                                  the words { per row r: attacker bits | defender bits << 16 (king included) }, rep_ring[0..3], turn,
                                  attacker_reps | defender_reps << 16, side | attacker_mid_pair << 1 | defender_mid_pair << 2 | king row << 16 |
                                  king col << 20 - so the value of a leaf is a function of (seed, global game id, sim_offset, position) alone,
                                  as nnet.predict(canonicalBoard) of src/mcts.py:85 is a function of the board alone */
    uint32_t flags;            /* TAFL_MCTS_FLAG_* | tuning fields; 0 = src/mcts.py semantics, default pipeline */
} tafl_mcts_params;
/* semantics bits of tafl_mcts_params.flags.
 *   TAFL_MCTS_FLAG_FPU_INF  first-play urgency of the reference's Rust sketch, src/mcts.rs: an action that was never taken scores
 *     f64::INFINITY in the selection (mcts.rs:49-51), so every legal child of a node is expanded before any child is revisited, and a
 *     newly expanded node starts with visits = 1.0 instead of 0 (mcts.rs:187).  Ties keep src/mcts.py's rule (first maximum = lowest
 *     action index; the sketch does not compile and leaves the order of `valid_actions` undefined).  Everything else is src/mcts.py.
 *     This mode is pinned by the oracle only (no reference implementation can run it). */
#define TAFL_MCTS_FLAG_FPU_INF 0x1u
/*   TAFL_MCTS_FLAG_KEEP_TREE  continue the batch's retained tree instead of starting from an empty root: the reference's MCTS object with
 *     tables that persist across getActionProb calls (src/mcts.py:20-26).  A search of S followed by a keep-search of S' gives the result of
 *     one search of S + S', bit for bit; after tafl_mcts_advance the search starts from the played child's statistics.  Any other change to
 *     the batch (upload, reset_fen, step, step_kth, random_advance, a search without this bit, play_best, selfplay_run) drops the tree, and
 *     a keep-search on a dropped tree is a fresh search.  A kept leaf keeps the playout value it got in the search that expanded it; new
 *     leaves use this run's seed, sim_offset and ply cap.  tafl_selfplay_run rejects the bit. */
#define TAFL_MCTS_FLAG_KEEP_TREE 0x2u
/* tuning fields of tafl_mcts_params.flags: they choose HOW the same search is executed and never change its results
 * (tests/test_gpu_parity.py::test_mcts_pipelines_agree).
 *   bits 4-7   pipeline: 0 default (64-bit boards: fused; wider boards: two kernels per round, tree phase + playouts over dense work
 *              lists), 1 fused (one kernel per chunk of rounds, at most 2 playout slots per game; 64-bit boards only), 2 two-kernel
 *   bits 8-11  playout slots per game (one holds the pending simulation's leaf, the rest predicted leaves, DESIGN.md
 *              section 4.5); 0 = chosen from the batch size, at most 8
 *   bits 12-15 partitions of the batch that run the pipeline on their own streams (two-kernel pipeline); 0 = from the batch size, at most 8 */
#define TAFL_MCTS_PIPELINE_DEFAULT 0u
#define TAFL_MCTS_PIPELINE_FUSED 1u
#define TAFL_MCTS_PIPELINE_TWO_KERNEL 2u
#define TAFL_MCTS_TUNE_PIPELINE(x) (((uint32_t)(x) & 15u) << 4)
#define TAFL_MCTS_TUNE_SLOTS(x) (((uint32_t)(x) & 15u) << 8)
#define TAFL_MCTS_TUNE_PARTS(x) (((uint32_t)(x) & 15u) << 12)
#define TAFL_MCTS_TUNE_PARTS_OF(f) (((f) >> 12) & 15u)
#define TAFL_MCTS_TUNE_SHARE(x) (((uint32_t)(x) & 15u) << 16)     /* this search may fill 1/x of the device (0 = all of it): batches searched side by side */
#define TAFL_MCTS_TUNE_SHARE_OF(f) (((f) >> 16) & 15u)
#define TAFL_MCTS_TUNE_PIPELINE_OF(f) (((f) >> 4) & 15u)
#define TAFL_MCTS_TUNE_SLOTS_OF(f) (((f) >> 8) & 15u)
#define TAFL_MCTS_FLAGS_KNOWN 0x000FFFF3u

typedef struct tafl_mcts_stats {
    uint64_t sims;             /* simulations executed (all games) */
    uint64_t rollouts;         /* random playouts consumed by simulations (mispredicted speculative ones excluded) */
    uint64_t rollout_plies;    /* env steps inside playouts */
    uint64_t tree_depth_sum;   /* sum over sims of nodes on the selection path (d) */
    uint64_t children_scanned; /* sum over sims of visited children examined (for c-bar) */
    uint64_t terminal_hits;    /* sims that ended on a terminal tree node */
    uint64_t reason_hist[16];  /* playout terminations by reason (win reasons 0-6, draws 8-9, cap 14, stuck 15) */
    uint64_t faults;           /* games that raised a device-side fault flag */
    uint64_t spec_issued;      /* speculative playouts launched ahead of their simulation */
    uint64_t spec_hits;        /* ... of which were consumed by the simulation they were predicted for */
} tafl_mcts_stats;

typedef struct tafl_ctx   tafl_ctx;    /* rules + geometry + device + stream */
typedef struct tafl_batch tafl_batch;  /* n game states resident in HBM (+ optional MCTS arena) */

/* ---- context ---------------------------------------------------------------------------------
 * tafl_ctx_create replaces GameLogic::new(rules, board_length) (game/game/logic.rs:70-72).
 * word_bits selects the reference board word: 64 (SmallBasic, ROW_WIDTH 7), 128 (MediumBasic,
 * ROW_WIDTH 11) or 256 (LargeBasic, ROW_WIDTH 15) — game/board/state.rs:332-337.
 * `stream` is a hipStream_t to enqueue on, or NULL to let the library create one. */
int tafl_ctx_create(const tafl_rules* rules, uint8_t side_len, uint32_t word_bits, int device,
                    void* stream, tafl_ctx** out);
int tafl_ctx_destroy(tafl_ctx* ctx);
const char* tafl_last_error(void);
int tafl_abi_version(void);

/* Rule/board presets — game/preset.rs:12-124 (rules), :126-135 (boards).
 * names: "copenhagen", "brandubh", "magpie", "tablut", "koch". */
int tafl_preset_rules(const char* name, tafl_rules* out);
const char* tafl_preset_board(const char* name); /* start FEN, NULL if unknown; "copenhagen13" is build-defined */

/* dense action space (the `getActionSize()` of src/mcts.py:41): side_len^2 * 2*(side_len-1) actions — every
 * (from tile, destination on its row or column) pair.  For from = (r, c), n = side_len, dist >= 1:
 *   action = (r*n + c) * 2*(n-1) + slot,   slot = V+ (row+): dist-1            [n-1-r slots]
 *                                                 V- (row-): (n-1-r) + dist-1    [r slots]
 *                                                 H+ (col+): (n-1) + dist-1      [n-1-c slots]
 *                                                 H- (col-): (n-1) + (n-1-c) + dist-1   [c slots]
 * i.e. the iteration order of ValidPlayIterator (game/play.rs:157,166-183: V+,V-,H+,H-, distance ascending) over
 * iter_occupied (game/board/state.rs:202-216, row-major), so ascending action index == get_all_possible_moves
 * order (game/main.rs:33-43).  Dense mask: 2420 bits = 76 uint32 words for 11x11 (SURVEY.md §8d, M = 304 B). */
uint32_t tafl_action_size(const tafl_ctx* ctx);
uint32_t tafl_action_mask_words(const tafl_ctx* ctx);  /* uint32 words per game in a dense mask */
int tafl_action_encode(const tafl_ctx* ctx, tafl_play play, uint32_t* action);
int tafl_action_decode(const tafl_ctx* ctx, uint32_t action, tafl_play* play);

/* ---- batch of game states ---------------------------------------------------------------------
 * tafl_batch_reset_fen replaces GameState::new(fen, side) for every game (game/game/state.rs:136-145,
 * FEN grammar game/board/state.rs:225-250).  upload/download move whole GameState values. */
int tafl_batch_create(tafl_ctx* ctx, uint32_t n_games, tafl_batch** out);
int tafl_batch_destroy(tafl_batch* b);
uint32_t tafl_batch_size(const tafl_batch* b);
int tafl_batch_reset_fen(tafl_batch* b, const char* fen, uint8_t side_to_play);
int tafl_batch_upload(tafl_batch* b, const tafl_state* states, uint32_t first, uint32_t count);
int tafl_batch_download(tafl_batch* b, tafl_state* states, uint32_t first, uint32_t count);
int tafl_state_from_fen(const tafl_ctx* ctx, const char* fen, uint8_t side_to_play, tafl_state* out); /* host-only helper */
/* BoardState::to_fen (game/board/state.rs:271-295) of one state; returns the string length or a negative error (host only) */
int tafl_state_to_fen(const tafl_state* st, uint32_t word_bits, char* out, uint32_t cap);
int tafl_sync(tafl_ctx* ctx);

/* ---- hot path -----------------------------------------------------------------------------------
 * tafl_movegen: get_all_possible_moves (game/main.rs:33-43) = iter_occupied(side_to_play) x
 *   GameLogic::iter_plays (logic.rs:850-856, play.rs:139-226) for every game.
 *   out_counts[n] (host, may be NULL), out_masks[n * tafl_action_mask_words] (host, may be NULL):
 *   bit `action` set iff the play is legal.  Games that are over yield 0 plays (logic.rs:165-167).
 * tafl_validate: GameLogic::validate_play (logic.rs:219-222); out_codes[n] = TAFL_PLAY_*.
 * tafl_step: GameLogic::do_play (logic.rs:827-834) = validate + do_valid_play (:782-820);
 *   plays[n]; effects[n] may be NULL.  Invalid plays leave that game unchanged and set effects.code.
 * tafl_step_kth: same, but game i plays its (ranks[i] mod count)-th legal move in canonical order
 *   (BASELINE config 2); games with no legal move or already over are left unchanged (code GAME_OVER / NO_PIECE).
 * tafl_side_can_play: GameLogic::side_can_play (logic.rs:837-846) for `side`; out[n] = 0/1.
 * tafl_rollout: one seeded uniform-random playout per game from its current state WITHOUT
 *   modifying the batch (build-defined policy); results[n].
 * tafl_random_advance: game i plays plies[i] seeded random plies in place (config-2 input maker).
 */
int tafl_movegen(tafl_batch* b, uint32_t* out_counts, uint32_t* out_masks);
int tafl_validate(tafl_batch* b, const tafl_play* plays, uint8_t* out_codes);
int tafl_step(tafl_batch* b, const tafl_play* plays, tafl_effects* out_effects);
int tafl_step_kth(tafl_batch* b, const uint32_t* ranks, tafl_play* out_plays, tafl_effects* out_effects);
int tafl_side_can_play(tafl_batch* b, uint8_t side, uint8_t* out);
int tafl_rollout(tafl_batch* b, uint64_t seed, uint32_t sim, uint32_t max_plies,
                 uint64_t game_id_base, tafl_rollout_result* out_results);
int tafl_random_advance(tafl_batch* b, uint64_t seed, const uint32_t* plies, uint64_t game_id_base);

/* ---- MCTS -----------------------------------------------------------------------------------------
 * tafl_mcts_run replaces `for i in range(numMCTSSims): self.search(canonicalBoard)` of
 * MCTS.getActionProb (src/mcts.py:37-38) for every game of the batch, rooted at its current state,
 * with predict() = uniform priors + one seeded random playout (SURVEY.md §8a resolution):
 * select (mcts.py:104-123) / expand (:83-102) / rollout / backup (:127-136) as lock-step kernels.
 * The batch's states are not modified.  game_id_base is the global id of game 0 (RNG key), so
 * shards of a larger job reproduce the single-device results.
 * Results stay on the device until fetched:
 *   tafl_mcts_root_children: visited root edges in canonical order; out[n * max_children],
 *     out_n[n] = number of visited root children (<= max_children else TAFL_ERR_CAPACITY).
 *   tafl_mcts_root_visits: dense `counts` vector of mcts.py:41, out[n * tafl_action_size] uint32.
 *   tafl_mcts_policy: probs of mcts.py:40-53 (temp > 0: counts^(1/temp) normalised; temp == 0:
 *     one-hot on the FIRST maximum — the reference draws uniformly among maxima with np.random,
 *     the deterministic choice is documented in DESIGN.md); out[n * tafl_action_size] float64.
 *   tafl_mcts_best_play: max-visit root child (src/mcts.rs:216-227), first maximum.
 * tafl_mcts_reserve sizes the arena for searches of up to max_sims simulations ahead of time (tafl_mcts_run grows it by itself).  A
 * search in flight is joined first; the tree of the last search moves into the larger arena, so its readers (and a retained tree)
 * stay valid after the call.
 */
int tafl_mcts_reserve(tafl_batch* b, uint32_t max_sims);
int tafl_mcts_run(tafl_batch* b, const tafl_mcts_params* params, uint64_t game_id_base);
/* The same search without blocking the host (SURVEY 8b "calls enqueue ... asynchronous until tafl_sync"): tafl_mcts_run_async enqueues the
 * whole search on streams of the BATCH and returns; nothing is read back while it runs (plan and prediction width are steered on the
 * device).  tafl_mcts_wait joins it - and, while games are unfinished, runs the rounds its slowest games still need - so a search
 * always completes or the call fails.  tafl_mcts_run == tafl_mcts_run_async + tafl_mcts_wait; per-game results are identical.
 * Every reader of the results (root_children, root_visits, policy*, best_play, play_best, get_stats, round_trace) joins a search in
 * flight by itself.  One search per batch at a time (a second run_async first joins the first); DIFFERENT batches of one context search
 * side by side: the last rounds of a search are nearly empty (a few games whose simulations could not be predicted), and the device is
 * kept busy by another batch's full rounds.  tafl_mcts_run_async_after(b, ..., other) additionally holds b's search back until `other`'s
 * search in flight is half-way through its planned rounds (no effect if `other` has none): two half-size batches started this way stay
 * half a search apart, the steady state of a self-play loop `wait(A); play(A); run_async(A); wait(B); play(B); run_async(B)`.
 * A call that writes the batch states between run_async and wait (upload, reset_fen, step, step_kth, random_advance, mcts_play_best,
 * mcts_advance) joins the search first, as tafl_mcts_reserve does: the order {run_async; call} gives what {run; call} gives. */
int tafl_mcts_run_async(tafl_batch* b, const tafl_mcts_params* params, uint64_t game_id_base);
int tafl_mcts_run_async_after(tafl_batch* b, const tafl_mcts_params* params, uint64_t game_id_base, tafl_batch* other);
int tafl_mcts_wait(tafl_batch* b);
int tafl_mcts_get_stats(tafl_batch* b, tafl_mcts_stats* out);
int tafl_mcts_root_children(tafl_batch* b, tafl_root_child* out, uint32_t max_children, uint32_t* out_n);
int tafl_mcts_root_visits(tafl_batch* b, uint32_t* out);
int tafl_mcts_policy(tafl_batch* b, double temp, double* out);
int tafl_mcts_best_play(tafl_batch* b, tafl_play* out_plays, uint32_t* out_visits);
/* self-play step without leaving the device: every game plays the most visited root play of its last tafl_mcts_run (first maximum)
 * on its batch state (do_valid_play); finished games are left alone (effects.code = TAFL_PLAY_GAME_OVER).  out_* may be NULL
 * (then nothing is copied back and the call only enqueues). */
int tafl_mcts_play_best(tafl_batch* b, tafl_play* out_plays, tafl_effects* out_effects);
/* Self-play without leaving the device and without a barrier between the moves: for every game, n_moves times, a search of
 * params->n_sims simulations from its current state followed by its most visited root play (first maximum) on the batch state - per game
 * exactly `for m in 0..n_moves: tafl_mcts_run(sim_offset + m * n_sims); tafl_mcts_play_best` - but a game starts its next search as soon
 * as ITS OWN search is done, so the games of the batch are at different phases of their searches and the device stays full (a batch of
 * synchronous searches ends every search in a tail of nearly empty rounds).  Games that end stop searching; out_plays[m * n + g] (may be
 * NULL) is the play game g made at move m, all-zero once its game was over.  tafl_mcts_get_stats afterwards covers all searches: a game
 * that ends inside the run is not searched again, and a game that is already over when the run begins is searched ONCE from its terminal
 * root (n_sims simulations, all of them terminal_hits, as tafl_mcts_run books them), makes no play and stops - so an episode played in
 * several runs books n_sims more `sims` per finished game and run than the same episode in one run; plays, states and examples are the same. */
int tafl_selfplay_run(tafl_batch* b, const tafl_mcts_params* params, uint32_t n_moves, uint64_t game_id_base, tafl_play* out_plays);
/* Subtree reuse (TAFL_MCTS_FLAG_KEEP_TREE).  tafl_mcts_advance plays actions[g] (a dense action index, tafl_action_encode order) in game g
 * with do_valid_play, exactly as tafl_step, and makes the child (root, action) the root of the retained tree: every statistic below it is
 * kept, its siblings are dropped.  actions == NULL: the most visited root child, first maximum (tafl_mcts_play_best, but the tree is kept).
 * A game with nothing to play is left alone, its tree kept, its play all-zero and effects.code = TAFL_PLAY_GAME_OVER, as play_best
 * reports it: a TAFL_ACTION_NONE entry (even in an ongoing game), a game that is over, or (actions == NULL) a root without a visited
 * child.  A child that was never visited gives a fresh root.  An illegal action (action >= tafl_action_size: TAFL_PLAY_OUT_OF_BOUNDS)
 * leaves the state unchanged, drops the game's tree (a fresh root) and reports the validation code.
 * After an advance the readers (root_children, root_visits, policy*, best_play) report the kept root.  out_* may be NULL.  A search in
 * flight is joined first.
 * tafl_mcts_tree_nodes: nodes per game in the retained tree (out[n]) - the states of the reference's Es table below the root. */
#define TAFL_ACTION_NONE 0xFFFFFFFFu
int tafl_mcts_advance(tafl_batch* b, const uint32_t* actions, tafl_play* out_plays, tafl_effects* out_effects);
int tafl_mcts_tree_nodes(tafl_batch* b, uint32_t* out);

/* ---- training-tensor writers (the step right after the hot path) ------------------------------
 * tafl_encode_boards: board_to_matrix (game/main.rs:55-83) for every game: uint8 [n * side_len * side_len], row-major;
 *   corner tiles 20, throne 30, soldier +1, king +5 (no side distinction, as in the reference).
 * tafl_mcts_policy_device: the probs of src/mcts.py:40-53 written by a kernel, for any temp >= 0 (temp == 1: counts / sum, exact;
 *   temp == 0: one-hot on the first maximum); float64 [n * tafl_action_size].
 * `out` may be a host pointer (out_is_device = 0) or a device pointer of this ctx's device (out_is_device = 1, e.g. a
 * torch tensor's data_ptr): the second form never crosses PCIe. */
int tafl_encode_boards(tafl_batch* b, uint8_t* out, int out_is_device);
int tafl_mcts_policy_device(tafl_batch* b, double temp, double* out, int out_is_device);
/* the same with the choices mcts.py:44-45 leaves to np.random: temp == 0 puts the 1 on the floor(r * ties / 2^32)-th maximum in ascending action
 * order, r = taflmix32 word of (tie_seed, game_id_base + game); tie_seed == 0 = the first maximum.  Any temp >= 0: counts ** (1 / temp) is the
 * device math library's float64 pow (exact for temp == 1; within 4 ulp of the host's pow otherwise, tests/test_gpu_parity.py). */
int tafl_mcts_policy_device_ex(tafl_batch* b, double temp, uint64_t tie_seed, uint64_t game_id_base, double* out, int out_is_device);

/* ---- self-play that records training examples ---------------------------------------------------------------
 * What an AlphaZero loop takes from self-play: per move one example (board, side to move, search policy pi, result z) - executeEpisode of
 * alpha-zero-general, the code base src/mcts.py belongs to (the reference has no Coach) - left in HBM, and minibatches served from there.
 * It replaces the synchronous loop { tafl_mcts_run; tafl_mcts_policy_device + tafl_encode_boards; choose on the host; tafl_step }.
 *
 * tafl_selfplay_record is tafl_selfplay_run (same searches: sim_offset + m * n_sims, same seed, same ply cap, no barrier between the moves)
 * with two additions per game and move.  m = the move's number inside the run, M = opts->move_base + m its number in the episode,
 * gid = game_id_base + game, visited root edges in canonical (= ascending action) order, N = sum of their Nsa:
 *   the play   M >= temp_moves: the most visited child, first maximum - so temp_moves == 0 gives the plays and final states of
 *              tafl_selfplay_run bit for bit.  M < temp_moves: drawn in proportion to the visit counts (pi at temp = 1, src/mcts.py:50-52)
 *              in integers: r = ply_rand(sim_key(game_key(sample_seed, gid), M), 0) - the RNG words of the playouts -,
 *              k = (r * N) >> 32, and the play is the first child whose running sum of Nsa exceeds k.  No floating point, no dependence on
 *              the sharding.  A game that is over, or whose root has no visited child, plays nothing (all-zero play) and records nothing.
 *   the example, appended to `ex` (NULL: nothing is recorded, the plays are still drawn) when the game makes the move:
 *              the board_to_matrix bytes of the position BEFORE the play (what tafl_encode_boards writes), the side to move, the sparse
 *              policy (n_children and per visited root child (action, Nsa); dense pi is never stored), the dense action index of the
 *              play, and move_no = M.
 * Example j of game g has the index j * n_games + g; a game appends at len[g].  Capacity, decided by bookkeeping:
 *   ex->n_games != tafl_batch_size(b) (or another board size / device): TAFL_ERR_INVALID_ARG.
 *   len[g] == max_moves: the game keeps playing and records no more; counted in tafl_examples_stats.dropped.
 *   a root with more than max_children visited children: the example is written with n_children = 0 (its gather row is all zero), counted
 *   in tafl_examples_stats.overflowed, and the game goes on.  A search of S simulations visits fewer than S root children, so
 *   max_children >= n_sims can never overflow.  Neither is a fault of the search: tafl_mcts_stats.faults does not count them.
 * n_sims must be below 65536.  TAFL_MCTS_FLAG_KEEP_TREE and the fused pipeline are rejected as tafl_selfplay_run rejects them
 * (TAFL_ERR_UNSUPPORTED); opts->flags and the reserved words must be 0 (TAFL_ERR_UNSUPPORTED).  tafl_mcts_get_stats covers all searches.
 *
 * tafl_examples_create: room for max_moves examples per game of n_games games, max_children (1..65535) policy entries each:
 *   n_games * max_moves * (4 * ceil(side_len^2 / 4) + 4 * max_children + 17) + 4 * n_games bytes on the context's device (the last term is
 *   the open_from array of tafl_gselfplay_begin_episodes; tafl_examples_stats.device_bytes counts it for every object).  The object outlives runs and
 *   batches (an episode may be played in several runs, move_base continuing the numbering); destroy it before its context.
 * tafl_examples_clear: every game back to 0 examples, the counters back to 0.
 * tafl_examples_counts: out_len[n_games] (may be NULL) and their sum (may be NULL).  tafl_examples_get_stats: the counters.
 * tafl_examples_finalize: one kernel that reads each game's CURRENT status from `b` (same size and device as `ex`; a search in flight on
 *   it is joined) and writes for every recorded example of that game z as float32 seen from the example's side to move: +1 that side
 *   won, -1 it lost, 1e-4 a draw (the value the search gives a drawn terminal), final = 1; examples of a game that is still going on get
 *   z = 0, final = 0, so the call can be repeated after the next run.
 *   Examples that an episodes run (tafl_gselfplay_begin_episodes) has closed or cut are left as that run wrote them.
 * tafl_examples_gather: minibatch rows.  For i < count, example index[i] under board symmetry sym[i] in 0..7 (sym == NULL: identity):
 *   boards[i * side_len^2 ..]  the board bytes, transformed;  sides[i], z[i], final_[i] copied;
 *   pi[i * tafl_action_size ..]  float32, zero except pi[sigma(action)] = (float)((double)Nsa / (double)N): the temp = 1 probs of
 *   src/mcts.py:50-52 rounded once to float32.  Any output pointer may be NULL.
 *   Symmetries (the eight of the square; every ruleset of this library is invariant under them): bit 2 of sym transposes (r, c) -> (c, r)
 *   first, then bit 0 mirrors the rows r -> n-1-r, then bit 1 mirrors the columns c -> n-1-c.  A board byte moves to the transformed tile;
 *   an action is transformed by transforming its from and to tiles and encoding them again (tafl_action_size above).
 *   ptrs_are_device = 0: all pointers are host pointers; an index that names no recorded example (or a sym above 7) fails the call with
 *   TAFL_ERR_INVALID_ARG before anything is written.  ptrs_are_device = 1: all pointers (index and sym included) are device pointers of
 *   the context's device, the kernel is enqueued on the context's stream (tafl_sync joins it) and nothing crosses PCIe; such an index
 *   gives an all-zero row and is counted in tafl_examples_stats.bad_index; sym is taken modulo 8.
 *
 * Search value and policy surprise (examples that carry search statistics).
 * tafl_examples_create_ex(ctx, n_games, max_moves, max_children, flags, out): flags = 0 is exactly tafl_examples_create.
 *   TAFL_EXAMPLES_SEARCH_STATS adds two float32 arrays cq and cp laid out like the policy words ([(j * K + k) * G + g], K = max_children,
 *   G = n_games): 8 * max_children bytes more per example, and 4 * n_games bytes of the recorder's bookkeeping, all counted in
 *   tafl_examples_stats.device_bytes.  Unknown flag bits: TAFL_ERR_UNSUPPORTED.  Without the flag nothing of this section is allocated,
 *   read, written or launched.
 * What is recorded: every guided self-play run (tafl_gselfplay_begin, _begin_episodes, tafl_gmatch_begin; with root noise, a playout cap -
 *   only full moves record -, forced playouts, the solver, an evaluation symmetry) that appends an example into such an object leaves,
 *   for every stored child k (the visited root edges in ascending action order, after solver and forced pruning: the counts are n'),
 *     cq[k] = (float)Qsa   and   cp[k] = (float)Ps[root][a]
 *   as the root's edge held them when the move was made.  The self-play rounds are what they were: one more kernel per round, one lane
 *   per game, reads the finished root's edge block, which stands until the next root is expanded.  Known and accepted: with root noise
 *   Ps is the MIXED prior (what tafl_gmcts_root_priors reports), and under an evaluation symmetry it is indexed by the original action.
 *   An example that overflowed or was dropped stores nothing.  tafl_examples_clear while a run records into the object is not supported.
 *   tafl_selfplay_record (rollout mode has no priors) refuses such an object: TAFL_ERR_UNSUPPORTED.
 * Two scalars per example, both 0 when the example has no stored policy (overflow, or no stored child):
 *   value:     N = sum of the Nsa;  acc = 0;  for k ascending: acc = acc + (double)Nsa_k * (double)cq_k;  value = (float)(acc / (double)N).
 *              No fused multiply-add: value is defined bit for bit.
 *   surprise:  pi_k = (double)Nsa_k / (double)N;  s = sum over k ascending, in double, of pi_k * (log(pi_k) - log(max((double)cp_k, 2^-126)));
 *              surprise = (float)max(s, 0.0).  This is KL(pi || P) over the stored children, in nats; it cannot be negative (log-sum
 *              inequality, the stored priors sum to at most 1) but for rounding.  `log` is the float64 logarithm of the device's math library.
 * tafl_examples_read_stats: q, prior [i * max_children + k] of the examples index[0 .. count) (0 beyond the stored children; either may
 *   be NULL).  Host pointers, the slow path of tafl_examples_read.  An index that names no recorded example, or an object without the
 *   flag: TAFL_ERR_INVALID_ARG.
 * tafl_examples_gather_stats: value[i], surprise[i] of example index[i], one kernel, one lane per row (either output may be NULL).  Host
 *   and device pointers as in tafl_examples_gather: a bad index fails the call with host pointers; with device pointers it writes zeros
 *   and is counted in tafl_examples_stats.bad_index.  An object without the flag: TAFL_ERR_INVALID_ARG.
 *   The training pool carries the two scalars and turns surprise into weights: tafl_pool_set_search_stats below.
 *
 * Value targets from search values (TD(lambda) per episode; the text of this block is normative).
 * TAFL_EXAMPLES_VALUE_TARGETS (with TAFL_EXAMPLES_SEARCH_STATS; alone: TAFL_ERR_UNSUPPORTED) adds per example one byte ep_end, one float32
 *   vt and one byte kind (6 bytes per example), and 32 bytes of result counters, all counted in device_bytes.  Without the flag nothing of
 *   this block is allocated, launched or read.
 * Episode boundaries: ep_end[j * G + g] = 1 iff j + 1 is a value the lane's open_from (the first example of its open episode: an episodes
 *   run sets it to the lane's example count whenever it closes or cuts an episode) has held since the last tafl_examples_clear while it was
 *   at or below the lane's example count.  One more kernel, one lane per game, marks it at the begin of a run and after every round and
 *   its reopen; the self-play rounds are what they were.  An episode without a recorded example leaves no mark; a lane of a run without
 *   episodes is one episode.
 * tafl_examples_value_targets(ex, cfg, out): per lane g the examples 0 .. min(len, max_moves) - 1 are split into episodes after every ep_end.
 *   An example takes part iff the N of its value (above) is > 0; the others get vt = 0, kind = 0 and are skipped.  For the participants
 *   i = 0 .. n-1 of one episode, ascending:  s_i = +1.0 if the side to move is TAFL_ATTACKER, else -1.0;  v_i = (double)value_i;
 *   u_i = s_i * v_i;  d_i = move_no_{i+1} - move_no_i clamped to 1 .. 65535.  The episode is closed iff final of its last participant is 1,
 *   otherwise unfinished (cut, or still open).
 *     lam_pow(d):  r = 1.0; b = lambda; for bit 0 .. 15: { if (d >> bit & 1) r = r * b;  b = b * b; }   (sixteen steps; lam_pow(1) == lambda)
 *     at i = n-1: A = 0.0, L = 1.0;  for i = n-2 down to 0:  p = lam_pow(d_i);  A = (1.0 - p) * u_{i+1} + p * A;  L = p * L
 *     T_i = closed ? (double)z_i : s_i * u_{n-1};   vt_i = (float)(s_i * A + L * T_i);   kind_i = closed ? 1 : 2
 *   All in float64 without fused multiply-add: vt is defined bit for bit.  lambda = 1 gives z on closed episodes and the last search
 *   value seen from the row's side on unfinished ones; lambda = 0 gives the next participant's value seen from the row's side.
 *   lambda outside [0, 1] (NaN included): TAFL_ERR_INVALID_ARG; unknown flag bits or non-zero reserved words: TAFL_ERR_UNSUPPORTED; an
 *   object without the flag: TAFL_ERR_INVALID_ARG.  out (may be NULL): episodes that hold a participant, closed and unfinished; the
 *   participants; the rows settled.
 *   TAFL_VT_SETTLE_UNFINISHED: the participants of unfinished episodes also get z_i = (float)(s_i * u_{n-1}) and final_i = 2, so that a
 *   following tafl_pool_ingest takes them (it takes final != 0) and tafl_examples_gather shows final = 2 for them.  A later
 *   tafl_examples_finalize rewrites the open tail from open_from on and undoes the settlement there.
 *   The result stands until tafl_examples_clear, tafl_examples_finalize or the begin - and every later round - of a run that records
 *   into the object, so the call belongs after the run (and, as for every recording run, the object must outlive the run: destroy it
 *   after tafl_gselfplay_end); then it is stale, and its readers (target and kind of tafl_examples_gather_targets, tafl_pool_ingest of a pool that carries targets) refuse it
 *   with TAFL_ERR_INVALID_ARG.
 * tafl_examples_gather_targets: target[i] = vt, kind[i], ep_end[i] of example index[i], one lane per row, any output may be NULL; host and
 *   device pointers and bad indices as in tafl_examples_gather_stats.  ep_end alone can be read while the result is stale. */
#define TAFL_EXAMPLES_SEARCH_STATS 0x1u          /* tafl_examples_create_ex: keep Qsa and Ps of every stored child */
#define TAFL_EXAMPLES_VALUE_TARGETS 0x2u         /* tafl_examples_create_ex: episode boundaries and a value target per example */
#define TAFL_VT_SETTLE_UNFINISHED 0x1u           /* tafl_value_targets_cfg.flags */
typedef struct tafl_value_targets_cfg { double lambda; uint32_t flags; uint32_t _reserved[5]; } tafl_value_targets_cfg;      /* 32 bytes */
typedef struct tafl_value_targets_result { uint64_t episodes_closed, episodes_unfinished, rows_with_target, rows_settled; } tafl_value_targets_result;   /* 32 bytes */
typedef struct tafl_examples tafl_examples;      /* opaque, owned by the ctx's device */
typedef struct tafl_selfplay_opts {
    uint64_t sample_seed;
    uint32_t temp_moves, move_base;
    uint32_t flags;                              /* 0 */
    uint32_t _reserved[3];
} tafl_selfplay_opts;                            /* 32 bytes */
typedef struct tafl_examples_stats {
    uint64_t dropped;        /* examples not recorded because their game already held max_moves */
    uint64_t overflowed;     /* examples recorded without a policy: more than max_children visited root children */
    uint64_t bad_index;      /* rows of device-pointer gathers whose index named no recorded example */
    uint64_t device_bytes;   /* device memory the object holds */
} tafl_examples_stats;                           /* 32 bytes */
int tafl_examples_create(tafl_ctx* ctx, uint32_t n_games, uint32_t max_moves, uint32_t max_children, tafl_examples** out);
int tafl_examples_destroy(tafl_examples* ex);
int tafl_examples_clear(tafl_examples* ex);
int tafl_examples_counts(tafl_examples* ex, uint32_t* out_len, uint64_t* out_total);
int tafl_examples_get_stats(tafl_examples* ex, tafl_examples_stats* out);
int tafl_selfplay_record(tafl_batch* b, const tafl_mcts_params* params, const tafl_selfplay_opts* opts, uint32_t n_moves,
                         uint64_t game_id_base, tafl_examples* ex, tafl_play* out_plays);
int tafl_examples_finalize(tafl_examples* ex, tafl_batch* b);
/* the sparse form of the examples index[0 .. count) (host pointers; an index that names no recorded example: TAFL_ERR_INVALID_ARG), for
 * hosts that store or inspect them: n_children[i], overflow[i] (1: more than max_children visited children, no policy stored), played[i]
 * (dense action index), move_no[i], and actions / visits [i * max_children + k] = the k-th visited root child in canonical order (0
 * beyond n_children).  Any output may be NULL.  It copies the arrays of the examples 0 .. max j asked for of every game to the host: not a hot path. */
int tafl_examples_read(tafl_examples* ex, const uint32_t* index, uint32_t count, uint32_t* n_children, uint8_t* overflow, uint32_t* played,
                       uint32_t* move_no, uint32_t* actions, uint32_t* visits);
int tafl_examples_gather(tafl_examples* ex, const uint32_t* index, const uint8_t* sym, uint32_t count,
                         uint8_t* boards, uint8_t* sides, float* pi, float* z, uint8_t* final_, int ptrs_are_device);
int tafl_examples_create_ex(tafl_ctx* ctx, uint32_t n_games, uint32_t max_moves, uint32_t max_children, uint32_t flags, tafl_examples** out);
int tafl_examples_read_stats(tafl_examples* ex, const uint32_t* index, uint32_t count, float* q, float* prior);
int tafl_examples_gather_stats(tafl_examples* ex, const uint32_t* index, uint32_t count, float* value, float* surprise, int ptrs_are_device);
int tafl_examples_value_targets(tafl_examples* ex, const tafl_value_targets_cfg* cfg, tafl_value_targets_result* out);
int tafl_examples_gather_targets(tafl_examples* ex, const uint32_t* index, uint32_t count, float* target, uint8_t* kind, uint8_t* ep_end, int ptrs_are_device);

/* ---- guided MCTS: src/mcts.py:55-136 with the CALLER's network as nnet.predict (mcts.py:85), SURVEY.md section 8f rank 3 ---
 * Lock-step over the batch: each tafl_gmcts_step (i) expands every waiting leaf with the priors / value the caller computed
 * for it (mask by the legal moves, renormalise with numpy's pairwise np.sum, all-masked workaround: mcts.py:86-98) and backs
 * the value up (mcts.py:127-136), then (ii) runs searches from the root until one reaches a state that needs predict();
 * searches that end in a terminal state are completed on the way.  A game is done after n_sims searches.
 *   priors  float32 [n * tafl_action_size], row g = network policy for game g's waiting leaf (rows of games that are not
 *           waiting are ignored); widened to float64 by the masking multiply as in mcts.py:87.
 *   values  float32 [n], used as Python floats (float(v)).
 *   first call after tafl_gmcts_begin: priors = values = NULL.  out_waiting (may be NULL) = games now waiting for predict().
 * tafl_gmcts_leaves: the network input for the waiting leaves: board_to_matrix planes uint8 [n * side_len * side_len]
 *   (game/main.rs:55-83), side to move [n] (TAFL_ATTACKER / TAFL_DEFENDER), waiting flag [n].
 * Device pointers (in_is_device / out_is_device = 1, e.g. torch tensors) keep the whole loop off PCIe.
 * tafl_gmcts_begin sizes the arena: max_sims + 1 nodes and (max_sims + 1) * edges_per_node edges per game (one edge per LEGAL
 * move of every expanded node); a game that outgrows it raises its fault flag and stops searching (stats.faults). */
typedef struct tafl_gmcts_stats {
    uint64_t sims, predicts, terminal_hits, faults, select_depth_sum, waiting, _reserved[2];
} tafl_gmcts_stats;                /* 64 bytes */
int tafl_gmcts_begin(tafl_batch* b, uint32_t max_sims, uint32_t edges_per_node);
int tafl_gmcts_step(tafl_batch* b, const float* priors, const float* values, int in_is_device, double c_puct, uint32_t n_sims,
                    uint32_t* out_waiting);
int tafl_gmcts_leaves(tafl_batch* b, uint8_t* boards, uint8_t* sides, uint8_t* waiting, int out_is_device);
int tafl_gmcts_root_children(tafl_batch* b, tafl_root_child* out, uint32_t max_children, uint32_t* out_n);
int tafl_gmcts_root_visits(tafl_batch* b, uint32_t* out, int out_is_device);
int tafl_gmcts_policy(tafl_batch* b, double temp, double* out, int out_is_device);
int tafl_gmcts_policy_ex(tafl_batch* b, double temp, uint64_t tie_seed, uint64_t game_id_base, double* out, int out_is_device);
int tafl_gmcts_get_stats(tafl_batch* b, tafl_gmcts_stats* out);
/* Subtree reuse in guided mode: tafl_gmcts_begin_ex(..., TAFL_GMCTS_KEEP_TREE) continues the retained tree (priors and values of kept nodes
 * stay; only new leaves wait for predict(), and stats.predicts counts only those), growing the arena by max_sims + 1 nodes beyond the kept
 * ones while keeping its contents; without the bit it is tafl_gmcts_begin.  tafl_gmcts_advance / tafl_gmcts_tree_nodes: the contract of
 * tafl_mcts_advance / tafl_mcts_tree_nodes on the guided tree.  The mutators listed at TAFL_MCTS_FLAG_KEEP_TREE and tafl_gmcts_begin drop it. */
#define TAFL_GMCTS_KEEP_TREE 0x1u
int tafl_gmcts_begin_ex(tafl_batch* b, uint32_t max_sims, uint32_t edges_per_node, uint32_t flags);
int tafl_gmcts_advance(tafl_batch* b, const uint32_t* actions, tafl_play* out_plays, tafl_effects* out_effects);
int tafl_gmcts_tree_nodes(tafl_batch* b, uint32_t* out);

/* ---- guided self-play at each game's own pace, recording training examples -------------------------------------
 * The network-guided twin of tafl_selfplay_record: every game, n_moves times, searches n_sims simulations with the CALLER's evaluator,
 * chooses its play, appends the move's example to `ex`, plays the move on its batch state and starts its next search in the same kernel
 * launch.  The host loop is  tafl_gselfplay_begin; tafl_gselfplay_step(NULL, NULL); while (waiting) { tafl_gmcts_leaves; network;
 * tafl_gselfplay_step(priors, values) }; tafl_gselfplay_end  - nothing is read back per move, and a game that finishes a search asks for
 * its next root's evaluation in the very next round, so the evaluator's batch stays full until games end.  It replaces, per move,
 * { tafl_gmcts_begin; the step loop; tafl_gmcts_root_visits to the host; a choice on the host; tafl_step }.
 *
 * Per game the run is exactly this loop (the evaluator must be a function of the leaf it is shown):
 *   for m in 0 .. n_moves:
 *       if the game is over: stop
 *       fresh root from the batch state                 (tafl_gmcts_begin)
 *       n_sims simulations of src/mcts.py:55-136        (the arithmetic of tafl_gmcts_step, unchanged)
 *       choose, record, play
 * with M = opts->move_base + m, gid = game_id_base + game, the visited root edges (Nsa > 0) in ascending action order, N = sum of their Nsa:
 *   choose     M >= temp_moves: the most visited edge, first maximum - what tafl_gmcts_advance(actions = NULL) plays.  M < temp_moves:
 *              r = ply_rand(sim_key(game_key(sample_seed, gid), M), 0), k = (r * N) >> 32, and the play is the first visited edge whose
 *              running sum of Nsa exceeds k: the word and the rule of tafl_selfplay_record.  No floating point, no dependence on the
 *              sharding.  A root without a visited edge (n_sims == 1) plays nothing and records nothing, and the game makes no further move.
 *   record     when ex != NULL, the example of tafl_selfplay_record: the board_to_matrix bytes of the position before the play, the side to
 *              move, n_children and per visited root edge (action, Nsa), the play's action, move_no = M.  The capacity rules are the same:
 *              len[g] == max_moves counts tafl_examples_stats.dropped, more than max_children visited edges counts overflowed (n_children =
 *              0); neither is a fault of the search.  tafl_examples_finalize and tafl_examples_gather are used as they are.
 *   play       do_valid_play on the batch state.  tafl_gselfplay_end hands out the plays [m * n + g] (all-zero for a move not made; may be
 *              NULL) and the number of moves each game made [n] (may be NULL).
 * A game whose arena overflows raises its fault flag as in tafl_gmcts_step (stats.faults), stops searching and moving, and the other
 * games are not affected.
 *
 * tafl_gselfplay_begin joins a search in flight, drops both retained trees, sizes the guided arena as tafl_gmcts_begin(n_sims,
 *   edges_per_node) does (a fresh root per move, no reuse), zeroes the guided stats and runs the first round; the first tafl_gselfplay_step
 *   then takes priors = values = NULL and reports the games that wait, exactly like tafl_gmcts_step after tafl_gmcts_begin (every later
 *   step takes both).  n_sims == 0, n_sims >= 65536, n_moves == 0, or `ex` of another size, board or device: TAFL_ERR_INVALID_ARG;
 *   non-zero opts->flags or reserved words: TAFL_ERR_UNSUPPORTED.
 * tafl_gselfplay_step: priors / values / in_is_device as tafl_gmcts_step; c_puct and n_sims are the run's.  out_waiting (may be NULL) == 0
 *   means the run is complete.  tafl_gmcts_leaves serves the network input unchanged; tafl_gmcts_get_stats covers all searches of the run.
 * A call that writes the batch states (tafl_batch_reset_fen, tafl_batch_upload, tafl_step, tafl_step_kth, tafl_random_advance,
 *   tafl_selfplay_run / _record, tafl_mcts_play_best, tafl_mcts_advance, tafl_gmcts_advance), a tafl_gmcts_begin / _begin_ex, or
 *   tafl_gselfplay_end closes the run: a tafl_gselfplay_step on a closed run fails with TAFL_ERR_INVALID_ARG.  tafl_gselfplay_end may be
 *   called while games still wait; the moves made so far stand. */
int tafl_gselfplay_begin(tafl_batch* b, uint32_t n_sims, uint32_t edges_per_node, double c_puct, const tafl_selfplay_opts* opts,
                         uint32_t n_moves, uint64_t game_id_base, tafl_examples* ex);
int tafl_gselfplay_step(tafl_batch* b, const float* priors, const float* values, int in_is_device, uint32_t* out_waiting);
int tafl_gselfplay_end(tafl_batch* b, tafl_play* out_plays, uint32_t* out_moves);

/* ---- guided self-play in episodes: a game that ends starts its next game in place ---------------------------------
 * tafl_gselfplay_begin_episodes opens a tafl_gselfplay run in which a lane does not idle once its game is over: the result is written to
 * the game's examples on the device, the lane takes its opening again under a new game id, and the new game's root waits for its
 * evaluation in the same round, so the evaluator's batch stays full.  tafl_gselfplay_step, tafl_gmcts_leaves, tafl_gselfplay_end and
 * tafl_gmcts_get_stats serve such a run as they serve a plain one.  Build-defined, like the run itself; its expectation is exact: episode k
 * of lane g equals the plain tafl_gselfplay_begin run from openings[g] with game_id_base + k * id_stride, move_base = 0 and the same seeds
 * and noise, truncated to the moves the lane had left or to episode_moves.
 *
 *   lane budget   n_moves is the lane's move budget over all its episodes; plays[m * n + g] and out_moves of tafl_gselfplay_end keep their
 *                 meaning (m counts the lane's moves, whichever episode they belong to).
 *   move numbers  are per episode and start at 0: opts->move_base must be 0 (TAFL_ERR_INVALID_ARG otherwise).
 *   openings      a batch of the same size, board and device as b (TAFL_ERR_INVALID_ARG otherwise); NULL or b itself: b's states at the
 *                 call.  Its states are copied into a buffer of b at the call: later writes to either batch do not change them.  Episode 0
 *                 of a lane begins from b's state, every later one from openings[g].
 *   episode k     of lane g has gid = game_id_base + k * id_stride + g (id_stride == 0 means n; a sharded caller passes the total number
 *                 of lanes) and M = the moves that episode has made.  Everything tafl_gselfplay_begin and tafl_root_noise key by (gid, M)
 *                 uses these: the word that draws a play, temp_moves, the example's move_no, the root-noise key.  The search, the pick,
 *                 the record and the play are those of tafl_gselfplay_begin, unchanged.
 *   close, reopen after a play, while the lane has budget left: an episode is CLOSED if its game is over, and CUT if it has made
 *                 episode_moves moves (0: no cap) and is still going.
 *                   closed: every example of the episode - indices open_from[g] .. len[g] of the lane's column - gets z by the rule of
 *                           tafl_examples_finalize from the final position and the example's side to move, and final = 1;
 *                   cut:    its examples keep z = 0, final = 0.
 *                 In both cases open_from[g] = len[g], the lane's episode count and one of the four counters of tafl_episode_stats go up,
 *                 the lane's batch state becomes its opening, k goes up by one, and the fresh root waits for its evaluation in this very
 *                 round: it is counted in out_waiting and served by tafl_gmcts_leaves.  At most one episode per lane is reopened per step.
 *                 A lane whose opening is not ongoing stops instead (its batch state stays the finished game).
 *   stops         a faulted lane, a lane without a visited root edge and a lane whose budget is used up stop as in a plain run.  A lane that
 *                 stops on its budget leaves its last episode OPEN - also when that game ended on the budget's last move: it is neither
 *                 counted nor settled by the run, and tafl_examples_finalize(ex, b) treats it as it treats a game of a plain run.
 *   capacity      `ex` holds max_moves examples per LANE, over all its episodes; dropped and overflowed are counted as before.
 * tafl_examples_finalize writes only the examples from open_from[g] on.  open_from is zero at tafl_examples_create and after
 *   tafl_examples_clear and only an episodes run moves it, so for an object that never saw one the call writes what it always wrote.
 *   tafl_examples_gather, _read and _counts are unchanged; an episode boundary in a lane's column is where move_no returns to 0 (in a run
 *   without a playout cap; with one, see tafl_playout_cap: move_no alone no longer shows it).
 * tafl_gselfplay_episode_stats: out_episodes[n] (may be NULL) = the episodes of each lane that were closed or cut, and the counters; valid
 *   from the begin until the next tafl_gselfplay_begin / _begin_episodes on the batch (TAFL_ERR_INVALID_ARG without an episodes run).
 * Non-zero eo->flags or reserved words: TAFL_ERR_UNSUPPORTED; eo == NULL: TAFL_ERR_INVALID_ARG; everything tafl_gselfplay_begin rejects is
 *   rejected alike, and what closes a plain run closes this one.  Not offered: continuing a cut or open episode in a later run. */
typedef struct tafl_episode_opts {
    uint64_t id_stride;        /* game id of episode k of lane g = game_id_base + k * id_stride + g; 0 means n */
    uint32_t episode_moves;    /* an episode that has made this many moves and is still going is cut (0: no cap) */
    uint32_t flags;            /* 0 */
    uint32_t _reserved[4];     /* 0 */
} tafl_episode_opts;           /* 32 bytes */
typedef struct tafl_episode_stats {
    uint64_t attacker_wins, defender_wins, draws;   /* closed episodes by result */
    uint64_t cut;                                   /* episodes cut at episode_moves */
    uint64_t _reserved[4];
} tafl_episode_stats;          /* 64 bytes */
int tafl_gselfplay_begin_episodes(tafl_batch* b, uint32_t n_sims, uint32_t edges_per_node, double c_puct, const tafl_selfplay_opts* opts,
                                  uint32_t n_moves, uint64_t game_id_base, tafl_examples* ex, const tafl_episode_opts* eo, tafl_batch* openings);
int tafl_gselfplay_episode_stats(tafl_batch* b, uint32_t* out_episodes, tafl_episode_stats* out);

/* ---- match play: two evaluators play each other in an episodes run -----------------------------------------------
 * The step that decides whether a newly trained network replaces the old one: games between two evaluators, 0 and 1, colours alternating,
 * results tallied by seat.  A match run IS an episodes run - budget, openings, id_stride, episode_moves, temp_moves, sample_seed, examples,
 * closing and reopening all as tafl_gselfplay_begin_episodes defines them - in which every search is run with the evaluator that owns the
 * side to move at its root.  A guided search starts from a fresh root at every move, so there is no second tree: the device routes each
 * waiting leaf to its evaluator, hands each evaluator a dense batch of only its own leaves, reads the answers back by row and tallies.
 * Build-defined (the reference has no arena); alpha-zero-general's Arena is the model: each player searches with its own network, also at
 * the opponent's nodes inside its own search.
 *
 *   seat          in episode k of lane g, evaluator seat(g, k) = (game_id_base + g + k + swap) & 1 plays the attackers and the other one
 *                 the defenders; swap is 0 or 1.  Neighbouring lanes start with opposite colours, a lane alternates colours from episode to
 *                 episode, and the rule does not depend on the sharding (game_id_base + g is the lane's global number).
 *   owner         every leaf of a lane's current search is evaluated by owner(g) = (seat(g, k) + s) & 1, s = 0 if the attackers are to
 *                 move at the search's root and 1 if the defenders are.  The root is the lane's batch state.
 *   equivalence   a match run with the evaluators (f0, f1) leaves exactly what the tafl_gselfplay_begin_episodes run with the same
 *                 arguments leaves when that run's evaluator answers lane g's waiting leaf with f_owner(g)(leaf): the plays, the moves per
 *                 lane, the final batch states, every example field, z, final, open_from, tafl_episode_stats, the per-lane episode counts
 *                 and tafl_gmcts_stats.sims / predicts / terminal_hits / faults.  The search arithmetic, the pick rule, the record and
 *                 close / cut / reopen are untouched.
 *   root noise    evaluation matches do not use it: tafl_gmatch_begin fails with TAFL_ERR_UNSUPPORTED while root noise is set on the batch.
 *
 * The host loop is  tafl_gmatch_begin; for (;;) { tafl_gmatch_leaves; if both counts are 0: break; evaluator e on its count_e rows (e = 0, 1);
 * tafl_gmatch_step }; tafl_gselfplay_end; tafl_gmatch_get_stats.
 *
 * tafl_gmatch_begin does what tafl_gselfplay_begin_episodes does, first round included, and marks the run as a match.  Everything that call
 *   rejects is rejected alike; mo->swap > 1: TAFL_ERR_INVALID_ARG; non-zero mo->flags or reserved words: TAFL_ERR_UNSUPPORTED.
 * tafl_gmatch_leaves writes, for each evaluator e, a dense batch of its waiting leaves.  Row r of evaluator e is the r-th lane, in ascending
 *   lane order, that waits and has owner == e:  lanes[e][r] is that lane, boards[e][r * side_len^2 ..] and sides[e][r] are exactly what
 *   tafl_gmcts_leaves writes for that lane, and waiting[e][r] = (r < count_e) for every r < cap[e].  Rows at and beyond count_e of boards,
 *   sides and lanes are not written.  Any pointer of `io` may be NULL; out_is_device as in tafl_gmcts_leaves.  out_count gets the two
 *   counts: their sum is tafl_gmcts_stats.waiting, and both zero means the run is complete.  count_e > cap[e] (whichever pointers are
 *   given): TAFL_ERR_CAPACITY, nothing is written but out_count, and the call may be repeated; cap = the batch size is always enough.  The
 *   call also records each lane's row for the next step, in a buffer of the batch.
 * tafl_gmatch_step: priors[e] holds count_e rows of tafl_action_size float32 and values[e] count_e floats, in the row order of the preceding
 *   tafl_gmatch_leaves.  Host pointers: exactly count_e rows are staged; device pointers are used in place.  priors[e] and values[e] may be
 *   NULL when count_e == 0 (and are not read then).  A step without a successful tafl_gmatch_leaves since the last step or the begin:
 *   TAFL_ERR_INVALID_ARG.  It runs the round, the tally, and the close-and-reopen.
 * tafl_gmatch_get_stats: games[a][r] counts the episodes the run closed or cut while evaluator a played the attackers; r is attacker win,
 *   defender win, draw, cut - the four cases of tafl_episode_stats, and games[0][r] + games[1][r] equals that struct's field for every r.
 *   A game that ends on the lane's last budgeted move stays open and is not counted, as in an episodes run.  Valid from the begin until the
 *   next tafl_gselfplay_begin / _begin_episodes / tafl_gmatch_begin on the batch.
 * tafl_gselfplay_step on a match run, and tafl_gmatch_leaves / _step / _get_stats without a match run, fail with TAFL_ERR_INVALID_ARG.
 *   tafl_gmcts_leaves, tafl_gmcts_get_stats, tafl_gselfplay_episode_stats and tafl_gselfplay_end serve a match run as they serve an episodes
 *   run, and what closes an episodes run closes a match run.  Not offered: more than two evaluators, root noise, subtree reuse. */
typedef struct tafl_match_opts {
    uint32_t swap;             /* 0 or 1 */
    uint32_t flags;            /* 0 */
    uint32_t _reserved[6];     /* 0 */
} tafl_match_opts;             /* 32 bytes */
typedef struct tafl_match_io {
    uint8_t*  boards[2];       /* [cap[e] * side_len^2] */
    uint8_t*  sides[2];        /* [cap[e]] */
    uint8_t*  waiting[2];      /* [cap[e]] */
    uint32_t* lanes[2];        /* [cap[e]] */
    uint32_t  cap[2];          /* rows each evaluator's buffers hold */
} tafl_match_io;
typedef struct tafl_match_stats {
    uint64_t games[2][4];      /* [evaluator that played the attackers][attacker win, defender win, draw, cut] */
    uint64_t _reserved[8];
} tafl_match_stats;            /* 128 bytes */
int tafl_gmatch_begin(tafl_batch* b, uint32_t n_sims, uint32_t edges_per_node, double c_puct, const tafl_selfplay_opts* opts, uint32_t n_moves,
                      uint64_t game_id_base, tafl_examples* ex, const tafl_episode_opts* eo, tafl_batch* openings, const tafl_match_opts* mo);
int tafl_gmatch_leaves(tafl_batch* b, const tafl_match_io* io, int out_is_device, uint32_t out_count[2]);
int tafl_gmatch_step(tafl_batch* b, const float* const priors[2], const float* const values[2], int in_is_device);
int tafl_gmatch_get_stats(tafl_batch* b, tafl_match_stats* out);

/* ---- Dirichlet noise at the root of a guided search --------------------------------------------------------------
 * AlphaZero's root exploration noise, P' = (1 - epsilon) P + epsilon eta with eta ~ Dir(alpha), for tafl_gmcts_* searches from fresh
 * roots and for tafl_gselfplay_* runs.  Build-defined (the reference has a TODO, src/mcts.rs:53).  Off by default; with it off nothing
 * in this header behaves differently.
 *
 * The root is node 0 of a fresh search.  After its priors P have been masked and normalised (mcts.py:86-98, the all-masked branch
 * included) let a_0 < ... < a_{n-1} be its legal actions in ascending dense order, gid = game_id_base + game, and M the move number: in a
 * tafl_gselfplay run opts->move_base + the moves the game has made in the run (and gid from that run's game_id_base), in a lock-step
 * search cfg->move_no (and cfg->game_id_base).
 *   words      w(i, k) = ply_rand(ak_i, k), the k-th uniform word of action a_i, with
 *                  mk   = sim_key(game_key(seed, gid) ^ 0x4449524943484C45, M)
 *                  ak_i = sim_key(mk | (uint64) fmix32(mk + 0x9E3779B9) << 32, a_i)
 *              (game_key / sim_key / ply_rand / fmix32 of the taflmix32 family).  The game key differs from the one selfplay_rand's word
 *              hangs off, so the two streams do not coincide for equal seeds.  A uniform is U(w0, w1) = ((w0 >> 5) * 2^26 + (w1 >> 6) + 0.5)
 *              * 2^-53, in (0, 1).
 *   gamma_i    one Gamma(alpha, 1) variate, a pure function of (seed, gid, M, a_i): not of n, the sharding or the lane.  Marsaglia-Tsang
 *              with shape k = alpha (alpha >= 1) or alpha + 1 (alpha < 1): d = k - 1/3, c = 1 / sqrt(9 d).  Round t = 0 .. 15 draws
 *              x = sqrt(-2 log U(w(i, 5t), w(i, 5t+1))) * cos(2 pi (w(i, 5t+2) + 0.5) 2^-32), u = U(w(i, 5t+3), w(i, 5t+4)), v = (1 + c x)^3 and
 *              accepts gamma = d v when v > 0 and log u < x^2 / 2 + d - d v + d log v.  If none of the 16 rounds accepts (probability below
 *              0.05^16 < 2e-21 per variate) gamma = d.  For alpha < 1 the result is multiplied by exp(log U(w(i, 80), w(i, 81)) / alpha),
 *              which may underflow to 0.  All in float64 with the math library of the side that runs it (device or host): the last bits of
 *              gamma are not portable between them, everything else here is.
 *   s          gamma_0 + gamma_1 + ..., summed sequentially in ascending action order in float64.
 *   eta_i      gamma_i / s; 1 / n if s is zero or not finite.
 *   mix        P'_i = (1.0 - epsilon) * P_i + epsilon * eta_i in float64: two multiplications and one addition, no FMA, no second
 *              renormalisation.
 * Only node 0 is mixed: the nodes below it are untouched, and a root that is terminal is never expanded and gets no noise.  PUCT, backup,
 * the pick rule, the example layout and the recorded visit counts are unchanged.
 *
 * tafl_gmcts_set_root_noise stores the setting on the batch (cfg == NULL: off).  tafl_gmcts_begin, tafl_gmcts_begin_ex and
 *   tafl_gselfplay_begin latch it: a change during a search or run takes effect at the next begin.  alpha not positive and finite, or
 *   epsilon outside (0, 1]: TAFL_ERR_INVALID_ARG; non-zero flags or _reserved: TAFL_ERR_UNSUPPORTED (the setting is left as it was).
 *   While noise is set, tafl_gmcts_begin_ex(TAFL_GMCTS_KEEP_TREE) fails with TAFL_ERR_UNSUPPORTED: a retained root is already expanded.
 * tafl_root_noise_eval is stateless and needs no search: for every game's current batch state it writes the dense row out_eta[g * A + a]
 *   (float64, A = tafl_action_size): eta at the legal actions, 0 elsewhere, all zero for a game that is over - exactly the values a
 *   search from that state under `cfg` mixes in (the same device function computes both).
 * tafl_gmcts_root_priors writes the dense Ps[root] [n * A] as the root's edges hold it (after the mix, if any); the row of a root that
 *   is not expanded is all zero. */
typedef struct tafl_root_noise {
    double   alpha;          /* > 0, finite */
    double   epsilon;        /* 0 < epsilon <= 1 */
    uint64_t seed;
    uint64_t game_id_base;   /* lock-step searches; a tafl_gselfplay run uses its own game_id_base */
    uint32_t move_no;        /* lock-step searches; a tafl_gselfplay run uses opts->move_base + m */
    uint32_t flags;          /* 0 */
    uint64_t _reserved;      /* 0 */
} tafl_root_noise;           /* 48 bytes */
int tafl_gmcts_set_root_noise(tafl_batch* b, const tafl_root_noise* cfg);
int tafl_root_noise_eval(tafl_batch* b, const tafl_root_noise* cfg, double* out_eta, int out_is_device);
int tafl_gmcts_root_priors(tafl_batch* b, double* out, int out_is_device);

/* ---- playout cap randomization in guided self-play ----------------------------------------------------------------
 * Most moves of a tafl_gselfplay run are searched cheaply, only to keep the game moving; a random minority is searched at full strength
 * and only those become training examples (KataGo's playout cap randomization).  Build-defined.  Off by default; with it off nothing in
 * this header behaves differently.  A lane whose move is fast finishes its search in fewer rounds and moves on inside the same launches.
 *
 * Let gid and M be the game id and the move number the run already uses for the word that draws a play and for the root-noise key: in a
 * plain run game_id_base + g and opts->move_base + the moves game g has made in the run, in an episodes run those of the lane's open
 * episode (game_id_base + k * id_stride + g and the moves that episode has made).
 *   class      w = ply_rand(sim_key(game_key(seed, gid) ^ 0x504C41594F555443, M), 0)  (the taflmix32 family; the constant keeps the stream
 *              apart from the sample stream and the noise stream when the seeds are equal).  The move is FULL iff (w >> 16) < full_per_65536,
 *              otherwise FAST: a pure function of (seed, gid, M), not of the lane, the sharding or what the run has done before.
 *              full_per_65536 = 65536 makes every move full, 0 makes every move fast.
 *   full move  the move as it is without a cap: n_sims simulations from a fresh root, root noise if the run latched it, the example is
 *              appended.
 *   fast move  fast_sims simulations from a fresh root.  No root noise, even when the run latched it.  No example is appended: len[g], the
 *              dropped and the overflowed counter are untouched.
 *   both       the play is chosen by the run's rule - for M < temp_moves the draw with the sample word of (gid, M), otherwise the most
 *              visited root edge, first maximum - and made on the batch state.  plays[m * n + g], out_moves, the lane budget,
 *              episode_moves, closing, cutting and reopening are unchanged: a fast move counts as a move everywhere.
 *   move_no    a recorded example keeps move_no = M.  Within an episode the recorded numbers increase but have gaps, and an episode may
 *              close having recorded nothing (then open_from[g] stays equal to len[g]).  With a cap an episode boundary in a lane's column
 *              can therefore NOT be read from move_no alone (it need not return to 0): use open_from, z / final and the episode counts.
 *   stats      tafl_gmcts_stats.sims counts the simulations actually run (n_sims per full move, fast_sims per fast one when nothing faults).
 *
 * tafl_gselfplay_set_playout_cap stores the setting on the batch (cfg == NULL: off).  tafl_gselfplay_begin and
 *   tafl_gselfplay_begin_episodes latch it: a change during a run takes effect at the next begin.  fast_sims < 2, fast_sims > 65535 or
 *   full_per_65536 > 65536: TAFL_ERR_INVALID_ARG; non-zero flags or _reserved: TAFL_ERR_UNSUPPORTED (in both cases the setting is left as
 *   it was).  A begin with fast_sims > n_sims fails with TAFL_ERR_INVALID_ARG and leaves no run open, so the arena stays sized by n_sims.
 *   While a cap is set tafl_gmatch_begin fails with TAFL_ERR_UNSUPPORTED.  The lock-step tafl_gmcts_* searches and the rollout-mode
 *   tafl_selfplay_record ignore the setting.
 * tafl_gselfplay_playout_cap_stats: the moves made per class, counted on the device when the move is made; valid from the begin until
 *   the next tafl_gselfplay_begin / _begin_episodes on the batch (also after tafl_gselfplay_end), TAFL_ERR_INVALID_ARG when that run
 *   latched no cap.
 * Not offered: recording fast moves, a cap in match runs or in rollout-mode self-play, subtree reuse (every move starts from a fresh root). */
typedef struct tafl_playout_cap {
    uint64_t seed;
    uint32_t fast_sims;        /* 2 .. n_sims of the run */
    uint32_t full_per_65536;   /* 0 .. 65536: a move is full with probability full_per_65536 / 65536 */
    uint32_t flags;            /* 0 */
    uint32_t _reserved[3];     /* 0 */
} tafl_playout_cap;            /* 32 bytes */
typedef struct tafl_playout_cap_stats { uint64_t full_moves, fast_moves, _reserved[2]; } tafl_playout_cap_stats;   /* 32 bytes */
int tafl_gselfplay_set_playout_cap(tafl_batch* b, const tafl_playout_cap* cfg);
int tafl_gselfplay_playout_cap_stats(tafl_batch* b, tafl_playout_cap_stats* out);

/* ---- forced playouts and policy target pruning in guided self-play ---------------------------------------------------
 * Root noise only changes priors: with few simulations a move the noise likes gets a visit or two and is never tested.  Forcing gives
 * every visited root child a minimum number of visits that grows with its (noised) prior; pruning then takes those visits out of the
 * recorded policy target wherever the search did not confirm them (KataGo's forced playouts with policy target pruning).  Build-defined.
 * Off by default; with it off nothing in this header behaves differently.
 *
 * All arithmetic is float64, in the order written, without contraction.  p, q, n are the fields of a root edge (Ps, Qsa, Nsa; for a move
 * that takes root noise p is the mixed prior), ns is the root's Ns, c_puct the run's.
 *   1 forcing   only at node 0 and only in the search of a FULL move (without a playout cap every move is full; a fast move of a capped
 *               run is neither forced nor pruned, as it takes no noise).  In the selection scan an edge with n > 0 and
 *               (double)n * (double)n < (k * p) * (double)ns scores +inf instead of its PUCT value.  The scan keeps its ascending action
 *               order and its strict >, so the first such edge is selected.  Every other node and edge keeps its arithmetic bit for bit.
 *   2 pruning   when the search of a full move is complete, before the play is chosen.  b = the first most visited root edge.
 *               sq = sqrt((double)ns);  U* = q_b + c_puct * p_b * sq / (double)(1 + n_b).  For every other visited edge j:
 *                 x = (k * p_j) * (double)ns;  F_j = the smallest integer F >= 0 with (double)F * (double)F >= x;
 *                 m = n_j; at most F_j times: stop if m == 0; if q_j + c_puct * p_j * sq / (double)(1 + (m - 1)) < U* then m -= 1, else stop;
 *                 after the walk, if m < n_j and m <= 1 then m = 0.
 *               The pruned count is n'_j = m; n'_b = n_b.
 *   3 after it  everything uses n': the visited-children count of the example (and its overflow test against max_children) is the number
 *               of edges with n' > 0, the stored (action | n' << 16) words and N = sum n' use n', for M < temp_moves the draw is the run's
 *               draw over n' with N' = sum n' (so the played action is among the stored children); the first-maximum pick is unchanged,
 *               since only other edges shrink.  A root with no visited edge behaves as without the setting.
 *
 * tafl_gselfplay_set_forced_playouts stores the setting on the batch (cfg == NULL: off).  tafl_gselfplay_begin and
 *   tafl_gselfplay_begin_episodes latch it: a change during a run takes effect at the next begin.  k not finite, k <= 0 or k > 64:
 *   TAFL_ERR_INVALID_ARG; non-zero flags or _reserved: TAFL_ERR_UNSUPPORTED (in both cases the setting is left as it was).  While it is
 *   set tafl_gmatch_begin fails with TAFL_ERR_UNSUPPORTED.  The lock-step tafl_gmcts_* searches (their getters included) and the
 *   rollout-mode tafl_selfplay_record ignore the setting.
 * tafl_gselfplay_forced_playouts_stats: forced_sims = simulations whose root selection was forced, pruned_visits = sum (n - n'),
 *   pruned_children = edges with n > 0 and n' == 0, full_moves = full moves made; counted on the device; valid from the begin until the
 *   next tafl_gselfplay_begin / _begin_episodes on the batch (also after tafl_gselfplay_end), TAFL_ERR_INVALID_ARG when that run latched
 *   no setting.
 * Not offered: forcing or pruning in lock-step searches, matches or rollout-mode self-play, the raw counts beside the pruned ones, a k
 *   that depends on the move, subtree reuse, temperatures other than 0 and 1. */
typedef struct tafl_forced_playouts {
    double k;                  /* 0 < k <= 64 (KataGo uses 2) */
    uint32_t flags;            /* 0 */
    uint32_t _reserved[5];     /* 0 */
} tafl_forced_playouts;        /* 32 bytes */
typedef struct tafl_forced_playouts_stats { uint64_t forced_sims, pruned_visits, pruned_children, full_moves; } tafl_forced_playouts_stats;   /* 32 bytes */
int tafl_gselfplay_set_forced_playouts(tafl_batch* b, const tafl_forced_playouts* cfg);
int tafl_gselfplay_forced_playouts_stats(tafl_batch* b, tafl_forced_playouts_stats* out);

/* ---- exact win/loss proofs in guided self-play: MCTS-Solver -----------------------------------------------------------
 * The game is decided by sudden tactics, and the one thing a search knows exactly is a finished game.  Without this setting a terminal
 * node is a value of +-1 averaged into a running mean; with it the search back-propagates PROOFS beside the values (Winands et al. 2008),
 * stops selecting moves that lose, ends as soon as its root is decided and keeps proven losses out of the play and the policy target.
 * Build-defined.  Off by default; with it off nothing in this header behaves differently.
 *
 * Every node has a proof: NONE, WON or LOST, for the side to move at that node.  All other arithmetic stays bit for bit: priors, PUCT,
 * the running-mean backup, the noise, the cap classes, the forcing.
 *   1 terminals    a node is created on the first visit of its edge.  If its game is over with a winner it is WON when the winner is the
 *                  side to move there, otherwise LOST; the backed-up value is -+term_value as without the setting.  A draw proves nothing.
 *   2 edges        an edge of node s is a LOSING MOVE once its child is WON, and a WINNING MOVE once its child is LOST.
 *   3 propagation  in the backup walk of every simulation, after the edge's Q/N update.  At each node s on the path whose proof is NONE:
 *                  s becomes WON if the child just left is LOST; s becomes LOST if that child is WON and every legal move of s has a child
 *                  that is WON (an unvisited edge has no child, so it blocks this).  The walk goes on to the root.
 *   4 selection    in a node whose proof is NONE the scan skips losing moves.  Everything else is unchanged: ascending action order, strict
 *                  >, and the +inf of tafl_forced_playouts rule 1 only for edges that are not skipped.  Such a node has at least one edge
 *                  that is no losing move and has no winning move.  A node whose proof is not NONE is never descended into (rule 5).
 *   5 the end      before each simulation: if the root's proof is not NONE the search of this move is complete - sims_done = n_sims,
 *                  kind = 3 - and the simulations not run are counted in skipped_sims (a fast move of a capped run counts from its own
 *                  n_sims - fast_sims).
 *   6 pruning      when the search of a move is complete, before rule 2 of tafl_forced_playouts and before the play is chosen; n' from n:
 *                  root WON: w = the first winning move in ascending action order, n'_w = n_w, every other n' = 0;
 *                  otherwise n' = 0 for every losing move, provided some edge that is not a losing move has n > 0; if none has (the
 *                  root is LOST, or only losing moves were visited) n' = n everywhere.
 *                  Afterwards everything uses n', exactly as rule 3 of tafl_forced_playouts says for its n': the forced-playouts pruning,
 *                  the children count and overflow test of the example, the stored (action | n' << 16) words, N, the draw for
 *                  M < temp_moves and the first-maximum pick.  So a WON root plays w whatever temp_moves is and records a one-entry
 *                  policy.  Fast moves are pruned too; they record nothing, as ever.
 * The proof of a node and the mark of an edge live in spare bits of the search arena; its sizes are those of a run without the setting.
 *
 * tafl_gselfplay_set_solver stores the setting on the batch (cfg == NULL: off).  tafl_gselfplay_begin and tafl_gselfplay_begin_episodes
 *   latch it: a change during a run takes effect at the next begin.  Non-zero flags or _reserved: TAFL_ERR_UNSUPPORTED (the setting is
 *   left as it was).  While it is set tafl_gmatch_begin fails with TAFL_ERR_UNSUPPORTED.  The lock-step tafl_gmcts_* searches (their
 *   getters included) and the rollout-mode tafl_selfplay_record ignore the setting.  It composes with root noise, the playout cap and
 *   forced playouts in every combination those allow.
 * tafl_gselfplay_solver_stats: root_won / root_lost = searches that were complete with a WON / LOST root, skipped_sims = simulations
 *   rule 5 did not run (tafl_gmcts_stats' sims + skipped_sims = the budgets of the searches), nodes_won / nodes_lost = non-root nodes that
 *   rule 3 marked (terminals are not counted), pruned_visits = sum (n - n') and pruned_children = edges with n > 0 and n' == 0 of rule 6,
 *   moves = moves made; counted on the device; valid from the begin until the next tafl_gselfplay_begin / _begin_episodes on the batch
 *   (also after tafl_gselfplay_end), TAFL_ERR_INVALID_ARG when that run latched no setting.
 * Not offered: proofs in lock-step searches, matches or rollout-mode self-play, subtree reuse, draw proofs, backing up proven values in
 *   place of the mean, a one-ply win check at expansion, transposition tables. */
typedef struct tafl_solver { uint32_t flags; uint32_t _reserved[7]; } tafl_solver;            /* 32 bytes, all 0 */
typedef struct tafl_solver_stats { uint64_t root_won, root_lost, skipped_sims, nodes_won, nodes_lost,
                                   pruned_visits, pruned_children, moves; } tafl_solver_stats;  /* 64 bytes */
int tafl_gselfplay_set_solver(tafl_batch* b, const tafl_solver* cfg);    /* NULL: off */
int tafl_gselfplay_solver_stats(tafl_batch* b, tafl_solver_stats* out);

/* ---- a random board symmetry per leaf evaluation in guided search and self-play ----------------------------------------
 * Every ruleset of this library is invariant under the eight symmetries of the square (tafl_examples_gather serves training rows under
 * them).  With this setting the evaluator is shown every leaf under a symmetry drawn for that leaf, and its policy is mapped back, as
 * AlphaZero and KataGo do: over the visits of a search the network's orientation bias averages out, at no cost to the evaluator.
 * Build-defined.  Off by default; with it off nothing in this header behaves differently and no new memory is read or written.
 *
 * Symmetry s (0 .. 7) is that of tafl_examples_gather: bit 2 transposes (r, c) -> (c, r) first, then bit 0 mirrors the rows, then bit 1
 * the columns; sym_tile(s, t) and sym_action(s, a) are its action on tiles and on dense actions (from and to tile transformed).
 *   the draw    for a leaf L that starts to wait for the evaluator in game g:  gid = game_id_base + g  (cfg's in a lock-step search, the
 *               run's own in a tafl_gselfplay_* run, as for root noise),  h = the leaf key of L (the state hash the playouts are keyed by),
 *                 s = ply_rand(sim_key(game_key(seed, gid) ^ 0x53594D4D45545259, h), 0) >> 29
 *               (the taflmix32 family).  A pure function of (seed, gid, position): not of the lane, the batch size, the sharding or the
 *               moment the search arrives, so the evaluator is still asked a function of the leaf it is shown, and a tafl_gselfplay run
 *               still equals its per-move loop.  The episode number is not part of the key: in an episodes run the start position of
 *               every episode of one lane draws the same s.
 *   the input   tafl_gmcts_leaves writes the board byte of tile t of a waiting leaf to tile sym_tile(s, t) of the game's row.  sides and
 *               waiting are unchanged, and so is the row of a game that does not wait.
 *   the answer  when the leaf is expanded the prior of its legal action a is read from priors_row[sym_action(s, a)].  Everything after that
 *               is unchanged and sees the legal actions in ascending original order: the masking multiply, the pairwise sum, the
 *               all-masked branch, the root-noise mix (keyed by the original action), PUCT, forced playouts, the solver, the recording.
 *               The value is used as delivered.
 * So the search equals mcts.py run with predict'(b) = (unpermute_s(P), v) where (P, v) = predict(transform_s(b)).
 *
 * tafl_gmcts_set_eval_symmetry stores the setting on the batch (cfg == NULL: off).  tafl_gmcts_begin, tafl_gmcts_begin_ex (with
 *   TAFL_GMCTS_KEEP_TREE too: the leaves of the continued search are drawn, the retained nodes keep their priors), tafl_gselfplay_begin and
 *   tafl_gselfplay_begin_episodes latch it: a change during a search or run takes effect at the next begin.  Non-zero flags or _reserved:
 *   TAFL_ERR_UNSUPPORTED (the setting is left as it was).  While it is set tafl_gmatch_begin fails with TAFL_ERR_UNSUPPORTED.
 * tafl_gmcts_leaf_symmetry writes out_sym[g] = s of the leaf of game g that waits now, 0 for a game that does not wait and for every game
 *   with the setting off [n bytes; out_is_device as in tafl_gmcts_leaves].  The step does not depend on this call or on tafl_gmcts_leaves.
 * Not offered: matches, averaging one leaf over several symmetries, symmetry in rollout-mode search, a draw keyed by the move or episode
 *   number, canonical positions. */
typedef struct tafl_eval_symmetry {
    uint64_t seed;
    uint64_t game_id_base;   /* lock-step searches; a tafl_gselfplay run uses its own game_id_base */
    uint32_t flags;          /* 0 */
    uint32_t _reserved[3];   /* 0 */
} tafl_eval_symmetry;        /* 32 bytes */
int tafl_gmcts_set_eval_symmetry(tafl_batch* b, const tafl_eval_symmetry* cfg);      /* NULL: off (the default) */
int tafl_gmcts_leaf_symmetry(tafl_batch* b, uint8_t* out_sym, int out_is_device);

/* ---- training pool: a window over finished examples, sampled on the device ------------------------------------------
 * The piece between "self-play wrote examples" and "the trainer takes a minibatch": a fixed-capacity ring of finished examples in HBM that
 * outlives the tafl_examples objects it was filled from (alpha-zero-general keeps the examples of the last N iterations and trains on
 * shuffled batches of them).  tafl_pool_ingest compacts the finished examples of an examples object into it, tafl_pool_sample draws rows
 * uniformly under random board symmetries, tafl_pool_sample_weighted in proportion to per-row integer weights the trainer hands back.
 * Build-defined.  Nothing else in this header behaves differently.
 *
 * Rows and slots.  A pool has `capacity` C rows (1 <= C < 2^32) of `max_children` Kp (1..65535) policy entries.  The q-th row ever taken
 *   (q from 0) lives in slot q mod C.  live = min(written, C) minus what tafl_pool_trim removed; the live rows are those with q in
 *   [written - live, written); a slot is live if and only if it holds one of them.  A row is contiguous: the ceil(side_len^2 / 4) board
 *   words of the example, n_children | side << 16, N, move_no, generation, z, Kp policy words action | Nsa << 16 in canonical order (zero
 *   beyond n_children), padded to a multiple of 16 bytes.  tafl_pool_create allocates
 *     capacity * 16 * ceil((ceil(side_len^2 / 4) + 5 + max_children) / 4) + 32 bytes
 *   on the context's device; the first ingest adds 16 bytes per 256 examples of room of the largest examples object ingested
 *   (n_games * max_moves), calls with host pointers add their staging; tafl_pool_stats.device_bytes counts all of it.  Destroy a pool
 *   before its context.
 * tafl_pool_ingest, as a serial loop over the per-example arrays of `ex` (G = n_games):
 *     T = 0
 *     for e = 0 .. G * max_moves - 1, ascending (j = e / G, g = e % G):
 *         if j >= min(len[g], max_moves): continue                       no example there
 *         if the example has the overflow mark: skipped_overflow += 1; continue
 *         if final == 0:                        skipped_open += 1;     continue
 *         rank[e] = T; T += 1
 *     generation = ingests + 1
 *     the example of rank r is written iff r >= T - min(T, C); its row number is q = written + r, its slot q mod C
 *     written += T; ingests += 1
 *   Examples with r < T - C are not stored at all, so no two stores of an ingest name the same slot.  The ranks come from a scan, not from
 *   atomics: the slot of every example is the one above on every run.  `ex` is not modified; ingesting it twice takes its examples twice
 *   (the documented use is tafl_examples_finalize or an episodes run, then tafl_pool_ingest, then tafl_examples_clear).  An ingest with
 *   T = 0 still counts as a generation.  `ex` of another context (hence another board size or device), or ex->max_children > Kp:
 *   TAFL_ERR_INVALID_ARG.  out (may be NULL) receives T and the two skip counts of this call.  The call is synchronous.
 *   Ordering: the ingest is enqueued on the context's stream.  That orders it after tafl_examples_finalize, after tafl_selfplay_record
 *   (which returns with its streams joined) and after every step of a guided run (tafl_gselfplay_*, tafl_gmatch_*) of a batch of the
 *   SAME context, open or ended.  A guided run of a batch of another context of the device writes `ex` on that context's stream: it
 *   must have been ended (tafl_gselfplay_end synchronises) before the ingest.  An examples object keeps no reference to the batches
 *   that record into it, so there is nothing an ingest could join.
 * tafl_pool_trim keeps only the rows of the newest keep_generations ingests (numItersForTrainExamplesHistory): bookkeeping on the host that
 *   lowers `live`; keep_generations == 0: TAFL_ERR_INVALID_ARG.  tafl_pool_clear empties the pool and zeroes all counters.
 * tafl_pool_sample: row i < count of the outputs uses row = row_base + i (a sum above 32 bits: TAFL_ERR_INVALID_ARG) and
 *     dk   = sim_key(game_key(seed, step) ^ 0x504F4F4C44524157, row)       the taflmix32 family of the playouts
 *     a    = (ply_rand(dk, 0) * live) >> 32                                age rank, 0 = the oldest live row
 *     slot = (written - live + a) mod C                                    64-bit arithmetic
 *     sym  = flags & TAFL_POOL_SAMPLE_SYM ? ply_rand(dk, 1) >> 29 : 0
 *   Integers only, a pure function of (seed, step, row, written, live, C): rank k of a data-parallel trainer passes row_base = k * count and
 *   the ranks together draw exactly the rows of one big call.  Row i is what tafl_pool_gather writes for (slot, sym); out_slot[i] and
 *   out_sym[i] (may be NULL) receive the draw.  live == 0: TAFL_ERR_INVALID_ARG; unknown flag bits: TAFL_ERR_UNSUPPORTED.
 * tafl_pool_gather: row i = the row in slot[i] under symmetry sym[i] (NULL: identity), exactly the bytes tafl_examples_gather wrote for the
 *   source example under that symmetry: boards[i * side_len^2 ..], sides[i], pi[i * tafl_action_size ..] with
 *   pi[sigma(action)] = (float)((double)Nsa / (double)N), z[i].  Any output pointer may be NULL.
 *   ptrs_are_device = 0 (both calls): host pointers; a slot that is not live or a sym above 7 fails the call with TAFL_ERR_INVALID_ARG
 *   before anything is written.  ptrs_are_device = 1: every pointer is a device pointer of the context's device, the kernel is enqueued on
 *   the context's stream (tafl_sync joins it) and nothing is read back; such a row is all zero and counted in tafl_pool_stats.bad_slot,
 *   sym is taken modulo 8.
 * tafl_pool_read: the sparse form of the rows in slot[0 .. count) (host pointers; a slot that is not live: TAFL_ERR_INVALID_ARG):
 *   n_children[i], move_no[i], generation[i], actions / visits [i * Kp + k].  Any output may be NULL.  It copies every row between the
 *   lowest and the highest slot asked for to the host: not a hot path.
 * Weighted sampling (off by default; while it is off the pool behaves and allocates as described above).  wt[s] is a uint32 per slot,
 *     eff(s) = slot s is live ? wt[s] : 0,   W(s) = sum of eff(t) for t < s, in SLOT order, 64 bits,   total = W(C).
 *   Slot order, not age order: the probability of a row is the same and the wrap of the window drops out of the search.  A weight left in
 *   a slot that is no longer live counts for nothing and needs no clearing.
 * tafl_pool_set_weighting(pool, w): w != NULL switches weighting on (flags or reserved words not 0: TAFL_ERR_UNSUPPORTED).  Off -> on
 *   allocates 4 bytes per slot (C rounded up to a multiple of 256), 20 bytes per 256 slots and 24 bytes, and gives EVERY slot
 *   w->ingest_weight; on -> on only changes ingest_weight for later ingests, stored weights stay.  w == NULL switches it off and frees
 *   those buffers and the staging of the weighted calls: tafl_pool_stats.device_bytes is what it was before (apart from row staging a
 *   weighted sample with host pointers grew, which is the staging of tafl_pool_sample).  tafl_pool_clear keeps the setting and the stored
 *   weights (no slot is live then).  While weighting is on, every row an ingest stores (ranks r >= T - min(T, C)) gets
 *   wt[slot] = ingest_weight.
 * tafl_pool_set_weights(pool, slot, weight, count, ptrs_are_device): afterwards every LIVE slot s named by the call holds the MAXIMUM of
 *   the weights the call gives for s (a sample with replacement names slots twice: the result does not depend on an order); slots not
 *   named are unchanged.  Weight 0 is legal: such a row is never drawn.  Host pointers: a slot that is not live fails the call with
 *   TAFL_ERR_INVALID_ARG before anything is written.  Device pointers: such an entry is skipped and counted in
 *   tafl_pool_weight_counters.bad_slot, the kernels are enqueued on the context's stream and nothing is read back.  Weighting off:
 *   TAFL_ERR_INVALID_ARG.  tafl_pool_get_weights reads weight[i] = wt[slot[i]]: a slot that is not live is refused with host pointers
 *   and reported as 0 with device pointers.
 * tafl_pool_sample_weighted: row i < count uses row = row_base + i (a sum above 32 bits: TAFL_ERR_INVALID_ARG) and
 *     dk   = sim_key(game_key(seed, step) ^ 0x504F4F4C57445257, row)       "POOLWDRW"
 *     r    = (uint64)ply_rand(dk, 2) << 32 | ply_rand(dk, 3)
 *     k    = (r * total) >> 64                                             128-bit product: k < total
 *     slot = the one s with W(s) <= k < W(s) + eff(s)
 *     sym  = flags & TAFL_POOL_SAMPLE_SYM ? ply_rand(dk, 1) >> 29 : 0
 *   Row i is what tafl_pool_gather writes for (slot, sym); out_slot[i], out_sym[i], out_weight[i] = wt[slot] and *out_total = total (one
 *   uint64; each may be NULL) receive the draw: a row's probability is wt / total, which is the caller's importance correction.  Integers
 *   only, a pure function of (seed, step, row, written, live, C, wt): ranks passing row_base = k * count draw the rows of one big call.
 *   Weighting off, live == 0 or total == 0: TAFL_ERR_INVALID_ARG; unknown flag bits: TAFL_ERR_UNSUPPORTED.  With device pointers every
 *   pointer (out_total too) is a device pointer.  tafl_pool_sample is untouched and ignores the weights.
 *   The sums behind the search are rebuilt in full (4 bytes read per slot) by the first weighted sample or tafl_pool_weight_stats after
 *   an ingest, a trim, a clear, tafl_pool_set_weights or tafl_pool_set_weighting; that rebuild reads 16 bytes back.
 * tafl_pool_weight_stats: enabled, ingest_weight, total_weight = total, positive = live rows with a weight above 0, bad_slot, rebuilds,
 *   device_bytes = what weighting added.  All zero while weighting is off; switching it off and tafl_pool_clear zero bad_slot and rebuilds.
 * Search statistics (off by default; while they are off the pool behaves and allocates as described above).
 * tafl_pool_set_search_stats(pool, on): allowed only while live == 0 (otherwise TAFL_ERR_INVALID_ARG).  On allocates two float32 arrays
 *   of `capacity` entries BESIDE the rows - value[s] and surprise[s] of the row in slot s; the row layout and the byte count of
 *   tafl_pool_create do not change, tafl_pool_stats.device_bytes counts the 8 * capacity bytes - off frees them.  tafl_pool_clear keeps
 *   the setting.  While it is on, tafl_pool_ingest refuses an examples object created without TAFL_EXAMPLES_SEARCH_STATS
 *   (TAFL_ERR_INVALID_ARG, nothing is taken) and runs one more pass that writes, for every row the ingest stores, the value and the
 *   surprise of its example - the two functions of tafl_examples_gather_stats, so a row's scalars equal what that call gives for its
 *   source example on the same device.  While it is off an ingest ignores the arrays of such an object.
 * tafl_pool_gather_stats: value[i], surprise[i] of the row in slot[i] (either may be NULL), with the rules of tafl_pool_get_weights for
 *   slots that are not live: refused with host pointers (TAFL_ERR_INVALID_ARG), zeros and counted in tafl_pool_stats.bad_slot with device
 *   pointers.  Search statistics off: TAFL_ERR_INVALID_ARG.
 * tafl_pool_weights_from_surprise(pool, cfg): needs weighting AND search statistics on (otherwise TAFL_ERR_INVALID_ARG); per_nat
 *   negative or NaN: TAFL_ERR_INVALID_ARG; flags or reserved words not 0: TAFL_ERR_UNSUPPORTED.  For every live slot s whose row has the
 *   generation cfg->generation (0: every live slot)
 *     x = (double)surprise[s] * per_nat;   wt[s] = min(2^32 - 1, base + (x < 2^32 ? (uint64)x : 2^32 - 1))
 *   which is an ASSIGNMENT, not the maximum rule of tafl_pool_set_weights; the other slots are unchanged.  One kernel over the slots on
 *   the context's stream, nothing is read back; the sums behind the weighted search are rebuilt by the next weighted sample, as after
 *   tafl_pool_set_weights.
 * Value targets (off by default).  tafl_pool_set_value_targets(pool, on): allowed only while live == 0 and only with search statistics on
 *   (otherwise TAFL_ERR_INVALID_ARG).  On allocates float32 vt[capacity] and uint8 kind[capacity] beside the rows; device_bytes counts the
 *   5 * capacity bytes, the row layout does not change, tafl_pool_clear keeps the setting, switching search statistics off switches it
 *   off too.  While it is on, tafl_pool_ingest refuses (TAFL_ERR_INVALID_ARG, nothing is taken) an examples object without
 *   TAFL_EXAMPLES_VALUE_TARGETS or whose targets are stale, and one more pass of its own (the rank and the placement of the pass that
 *   writes value and surprise) copies vt and kind of every row the ingest stores.  A trim and a wrap treat the two arrays as they treat value and surprise.
 * tafl_pool_gather_targets: target[i], kind[i] of the row in slot[i] (either may be NULL), with the rules of tafl_pool_gather_stats for
 *   slots that are not live.  The setting off: TAFL_ERR_INVALID_ARG.
 * De-duplication of positions (nothing of it exists until the first tafl_pool_dedup; the rows of the ring are never moved or merged).
 * tafl_pool_dedup(pool, cfg, out) groups the live rows [written - live, written) as they are at the call.  For a row with board bytes
 *   b[t], t < n^2 (n = side_len) and side to move `side` (TAFL_ATTACKER / TAFL_DEFENDER as tafl_pool_gather writes it):
 *     image(sigma)  has byte b[t] at tile sym_tile(sigma, t) (the symmetry of tafl_examples_gather), packed four tiles per 32-bit word -
 *                   tile u is byte u & 3 of word u >> 2 - with zero bytes beyond n^2: BW = ceil(n^2 / 4) words w_0 .. w_{BW-1}
 *     h(sigma)      x = 0x9E3779B97F4A7C15 ^ side;  for i = 0 .. BW-1: x = mix64(x ^ w_i)              (64-bit, wrapping)
 *     mix64(x)      x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31   (the splitmix64 finaliser)
 *     without TAFL_POOL_DEDUP_SYMMETRIES  key = h(0), canon = 0
 *     with it                             key = min over sigma in 0..7 of h(sigma), canon = the smallest sigma that attains the minimum
 *     then key &= 2^key_bits - 1 (cfg->key_bits in 1..64; 0 means 64), and a key of 0 becomes 1.
 *   key_bits below 64 makes keys collide on purpose: it is how the colliding path is tested and how collisions can be measured.
 *   Rows with equal keys form a group.  Of a group: m = its size; rep = the slot of its newest member (the largest age rank
 *   (s - first + C) mod C, first = (written - live) mod C); wins / losses = its members with z == 1.0f / z == -1.0f;
 *     zmean = (float)(((double)wins - (double)losses + (double)(m - wins - losses) * (double)(float)1e-4) / (double)m)
 *   (1e-4 is z of a drawn game).  Kept beside the rows, per live slot s: rep[s], mult[s] = m, zmean[s].  They are pure functions of the
 *   pool's contents: the groups are built from integer sums and maxima alone, no output depends on the order in which anything ran.
 *   *out (may be NULL): live, distinct = the number of groups, largest = the largest m, collisions = the live rows whose side or canonical
 *   image (the image under their own canon) differs from their representative's - expected to be 0 at 64 bits, a caller can check it -
 *   and device_bytes = what de-duplication added to tafl_pool_stats.device_bytes.  The buffers are allocated by the first call and sized
 *   for the capacity C: 25 * C bytes (rep, mult, zmean, the index of the row's table entry: 4 each; key: 8; canon: 1), a table of 24 bytes
 *   per entry with TS(C) entries, TS(x) = the power of two >= max(64, 2 * x), 32 bytes of results, and the staging of host-pointer
 *   tafl_pool_gather_dedup calls (16 bytes per row).  A call clears and uses TS(live) entries.  One 32-byte read-back per call.
 *   Errors: unknown flag bits, key_bits > 64 or reserved words not 0: TAFL_ERR_UNSUPPORTED; live == 0: TAFL_ERR_INVALID_ARG; a capacity
 *   above 2^30: TAFL_ERR_UNSUPPORTED.  cfg == NULL frees everything de-duplication allocated (tafl_pool_stats.device_bytes is what it was
 *   before the first call) and drops the result; *out is zeroed.
 *   The result stands until the next tafl_pool_ingest, tafl_pool_trim or tafl_pool_clear (whatever they change); after one of those
 *   tafl_pool_gather_dedup and tafl_pool_weights_from_dedup return TAFL_ERR_INVALID_ARG until the next tafl_pool_dedup.
 * tafl_pool_gather_dedup: rep[i], mult[i], zmean[i] of the row in slot[i] (any output may be NULL), with the rules of
 *   tafl_pool_gather_stats for slots that are not live: refused with host pointers before anything is written (TAFL_ERR_INVALID_ARG),
 *   zeros and counted in tafl_pool_stats.bad_slot with device pointers.
 * tafl_pool_weights_from_dedup(pool, cfg): needs weighting on and a result that stands (otherwise TAFL_ERR_INVALID_ARG); unknown flag
 *   bits, both flags together or reserved words not 0: TAFL_ERR_UNSUPPORTED.  For every live slot s, an ASSIGNMENT as in
 *   tafl_pool_weights_from_surprise (integer division):
 *     flags == 0                            wt[s] = max(1, scale / mult[s])         every distinct position is drawn equally often
 *     TAFL_POOL_DEDUP_DIVIDE                wt[s] = wt[s] == 0 ? 0 : max(1, wt[s] / mult[s])     keeps the weights, spreads them over the group
 *     TAFL_POOL_DEDUP_REPRESENTATIVES       wt[s] = rep[s] == s ? scale : 0         the newest search's policy, to be trained with zmean
 *   One kernel over the slots on the context's stream, nothing is read back; the sums behind the weighted search are rebuilt by the next
 *   weighted sample.
 * Not offered: saving and loading a pool, sampling without replacement, float weights,
 *   merging the policies of a group into one row, removing duplicate rows from the ring, de-duplication at ingest, groups across pools
 *   or devices, ingesting examples that are not final, a pool that spans devices, surprise over unvisited children,
 *   decay of weights by generation. */
typedef struct tafl_pool tafl_pool;                 /* opaque, owned by the ctx's device */
typedef struct tafl_pool_stats {
    uint64_t written;          /* rows ever taken by ingests (also those that fell out of the window) */
    uint64_t live;             /* rows that can be sampled now */
    uint64_t ingests;          /* tafl_pool_ingest calls that succeeded = the newest generation */
    uint64_t oldest_generation;/* generation of the oldest live row (0: empty) */
    uint64_t skipped_open;     /* over all ingests: recorded examples with final == 0 */
    uint64_t skipped_overflow; /* over all ingests: recorded examples with the overflow mark (no policy) */
    uint64_t bad_slot;         /* rows of device-pointer gathers whose slot was not live */
    uint64_t device_bytes;
} tafl_pool_stats;                                  /* 64 bytes */
typedef struct tafl_pool_ingest_result { uint64_t taken, skipped_open, skipped_overflow, _reserved; } tafl_pool_ingest_result;   /* 32 bytes */
#define TAFL_POOL_SAMPLE_SYM 0x1u   /* draw one of the eight symmetries per row; without it sym = 0 */
int tafl_pool_create(tafl_ctx* ctx, uint32_t capacity, uint32_t max_children, tafl_pool** out);
int tafl_pool_destroy(tafl_pool* pool);
int tafl_pool_clear(tafl_pool* pool);
int tafl_pool_get_stats(tafl_pool* pool, tafl_pool_stats* out);
int tafl_pool_ingest(tafl_pool* pool, tafl_examples* ex, tafl_pool_ingest_result* out);
int tafl_pool_trim(tafl_pool* pool, uint32_t keep_generations);
int tafl_pool_sample(tafl_pool* pool, uint64_t seed, uint64_t step, uint32_t row_base, uint32_t count, uint32_t flags,
                     uint8_t* boards, uint8_t* sides, float* pi, float* z, uint32_t* out_slot, uint8_t* out_sym, int ptrs_are_device);
int tafl_pool_gather(tafl_pool* pool, const uint32_t* slot, const uint8_t* sym, uint32_t count,
                     uint8_t* boards, uint8_t* sides, float* pi, float* z, int ptrs_are_device);
int tafl_pool_read(tafl_pool* pool, const uint32_t* slot, uint32_t count, uint32_t* n_children, uint32_t* move_no,
                   uint32_t* generation, uint32_t* actions, uint32_t* visits);
typedef struct tafl_pool_weights {
    uint32_t ingest_weight;    /* the weight of every slot at off -> on, and of every row an ingest stores */
    uint32_t flags;            /* 0 */
    uint32_t _reserved[6];     /* 0 */
} tafl_pool_weights;                                /* 32 bytes */
typedef struct tafl_pool_weight_counters {
    uint64_t enabled;          /* 1 while weighting is on; every other field is 0 while it is off */
    uint64_t ingest_weight;
    uint64_t total_weight;     /* the sum of the weights of the live rows */
    uint64_t positive;         /* live rows with a weight above 0 */
    uint64_t bad_slot;         /* entries of device-pointer tafl_pool_set_weights calls whose slot was not live */
    uint64_t rebuilds;         /* rebuilds of the sums behind the search */
    uint64_t device_bytes;     /* what weighting added to tafl_pool_stats.device_bytes */
    uint64_t _reserved;
} tafl_pool_weight_counters;                        /* 64 bytes */
int tafl_pool_set_weighting(tafl_pool* pool, const tafl_pool_weights* w);             /* NULL: off (the default) */
int tafl_pool_set_weights(tafl_pool* pool, const uint32_t* slot, const uint32_t* weight, uint32_t count, int ptrs_are_device);
int tafl_pool_get_weights(tafl_pool* pool, const uint32_t* slot, uint32_t count, uint32_t* weight, int ptrs_are_device);
int tafl_pool_sample_weighted(tafl_pool* pool, uint64_t seed, uint64_t step, uint32_t row_base, uint32_t count, uint32_t flags,
                              uint8_t* boards, uint8_t* sides, float* pi, float* z, uint32_t* out_slot, uint8_t* out_sym,
                              uint32_t* out_weight, uint64_t* out_total, int ptrs_are_device);
int tafl_pool_weight_stats(tafl_pool* pool, tafl_pool_weight_counters* out);
typedef struct tafl_pool_surprise_weights {
    uint32_t base;             /* the weight of a row without surprise */
    uint32_t generation;       /* only the rows of this ingest; 0: every live row */
    double per_nat;            /* weight added per nat of surprise, >= 0 */
    uint32_t flags;            /* 0 */
    uint32_t _reserved[3];     /* 0 */
} tafl_pool_surprise_weights;                       /* 32 bytes */
int tafl_pool_set_search_stats(tafl_pool* pool, int on);                              /* 0: off (the default) */
int tafl_pool_gather_stats(tafl_pool* pool, const uint32_t* slot, uint32_t count, float* value, float* surprise, int ptrs_are_device);
int tafl_pool_weights_from_surprise(tafl_pool* pool, const tafl_pool_surprise_weights* cfg);
int tafl_pool_set_value_targets(tafl_pool* pool, int on);                             /* 0: off (the default) */
int tafl_pool_gather_targets(tafl_pool* pool, const uint32_t* slot, uint32_t count, float* target, uint8_t* kind, int ptrs_are_device);
#define TAFL_POOL_DEDUP_SYMMETRIES 0x1u        /* tafl_pool_dedup: positions that are images of each other under a board symmetry are one group */
typedef struct tafl_pool_dedup_cfg {
    uint32_t flags;            /* 0 or TAFL_POOL_DEDUP_SYMMETRIES */
    uint32_t key_bits;         /* bits of the hash that make the key, 1..64; 0: 64 */
    uint32_t _reserved[6];     /* 0 */
} tafl_pool_dedup_cfg;                              /* 32 bytes */
typedef struct tafl_pool_dedup_result {
    uint64_t live;             /* the rows the call looked at */
    uint64_t distinct;         /* groups */
    uint64_t largest;          /* members of the largest group */
    uint64_t collisions;       /* live rows whose side or canonical image differs from their representative's */
    uint64_t device_bytes;     /* what de-duplication added to tafl_pool_stats.device_bytes */
    uint64_t _reserved[3];
} tafl_pool_dedup_result;                           /* 64 bytes */
#define TAFL_POOL_DEDUP_DIVIDE 0x1u            /* tafl_pool_weights_from_dedup: divide the weight a row has by its group's size */
#define TAFL_POOL_DEDUP_REPRESENTATIVES 0x2u   /* tafl_pool_weights_from_dedup: `scale` for the newest row of a group, 0 for the others */
typedef struct tafl_pool_dedup_weights {
    uint32_t scale;            /* the weight of a distinct position (flags 0) or of a representative */
    uint32_t flags;            /* 0, TAFL_POOL_DEDUP_DIVIDE or TAFL_POOL_DEDUP_REPRESENTATIVES */
    uint32_t _reserved[6];     /* 0 */
} tafl_pool_dedup_weights;                          /* 32 bytes */
int tafl_pool_dedup(tafl_pool* pool, const tafl_pool_dedup_cfg* cfg, tafl_pool_dedup_result* out);       /* cfg NULL: free */
int tafl_pool_gather_dedup(tafl_pool* pool, const uint32_t* slot, uint32_t count, uint32_t* rep, uint32_t* mult, float* zmean, int ptrs_are_device);
int tafl_pool_weights_from_dedup(tafl_pool* pool, const tafl_pool_dedup_weights* cfg);

/* ---- replay buffer on disk: write_to_file, game/main.rs:86-132 ------------------------
 * Host-only, byte-exact text format of the reference: per record `side_len` lines of comma-separated matrix values, one line
 * with the comma-separated vector, one line value1, one line value2; every line ends in '\n'.
 * FIFO rule exactly as the reference implements it: the existing file is split into LINES, and if their number is
 * >= max_entries ONE line (the first) is dropped before the new record is appended (main.rs:98-106) — the cap counts lines,
 * not records.
 *   tafl_replay_append        one record (one write_to_file call).
 *   tafl_replay_append_batch  n records, identical to n consecutive tafl_replay_append calls in order, with one read and one
 *                             write of the file.  matrices[n*side_len*side_len]; record g's vector is
 *                             vectors[vector_offsets[g] .. vector_offsets[g+1]).
 *   tafl_replay_read          (the reference has no reader) the newest <= max_records complete records, oldest first, parsed
 *                             from the end of the file; vectors[k*vector_cap ..], vector_lens[k].  Any output may be NULL. */
int tafl_replay_append(const char* path, const uint8_t* matrix, uint8_t side_len, const uint8_t* vector, uint32_t vector_len,
                       uint8_t value1, uint8_t value2, uint64_t max_entries);
int tafl_replay_append_batch(const char* path, const uint8_t* matrices, uint8_t side_len, uint32_t n, const uint8_t* vectors,
                             const uint32_t* vector_offsets, const uint8_t* values1, const uint8_t* values2, uint64_t max_entries);
int tafl_replay_read(const char* path, uint8_t side_len, uint32_t max_records, uint8_t* matrices, uint8_t* vectors, uint32_t vector_cap,
                     uint32_t* vector_lens, uint8_t* values1, uint8_t* values2, uint32_t* out_n);

/* ---- measurement helpers (bench.py) -----------------------------------------------------------------
 * HIP-event timing on the ctx stream: average duration of the named kernel class since the last reset.
 * classes: 0 movegen, 1 step, 2 rollout, 3 mcts tree step (k_mcts_tree), 4 mcts playouts (k_mcts_rollout / k_mcts_fused) */
int tafl_mcts_round_trace(tafl_batch* b, uint32_t* requested, uint32_t* run, uint32_t cap, uint32_t* n_rounds); /* playouts requested /
    run in each round of the last tafl_mcts_run (two-kernel pipeline; 0 rounds after a fused search); arrays may be NULL */
int tafl_timing_enable(tafl_ctx* ctx, int enable);
int tafl_timing_reset(tafl_ctx* ctx);
int tafl_timing_get(tafl_ctx* ctx, int kernel_class, double* total_ms, uint64_t* launches);
int tafl_timing_get_union(tafl_ctx* ctx, int kernel_class, double* union_ms, double* sum_ms);   /* time with >= 1 launch of the class
    in flight (launches on different streams overlap) and the plain sum of the launch durations, since the last reset */
void* tafl_ctx_stream(tafl_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* TAFLHIP_H */
