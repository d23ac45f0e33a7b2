/*
 * pmx.h -- C ABI of the MI355X-native Pac-Man Capture-the-Flag environment step.
 *
 * The reference (ceselder/pacman-marl-2025) is plain Python and has no FFI of its own; the boundary it
 * offers for this path is the call surface of gymPacMan.gymPacMan_parallel_env (gymPacMan.py:15-270) and
 * the CaptureAgent action API (captureAgents.py:91-162).  This header is the C ABI a maintainer would bind
 * UNDER those Python classes (ctypes stub in INTEGRATION.md); each entry point cites what it replaces.
 *
 * Conventions
 *   - every function returns 0 on success or a negative PMX_ERR_* code; pmx_last_error() returns a
 *     thread-local description of the last failure.  No exceptions cross the boundary.
 *   - the caller owns every buffer; the library owns only the opaque pmx_env handle (and the device
 *     memory behind it).  Pointers named *_dev are DEVICE pointers (HIP), everything else is host memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  All *_dev work is
 *     stream-ordered and asynchronous; the library never synchronises unless the comment says so.
 *   - a handle is bound to one device and is not thread-safe.
 *   - coordinates: (x, y), origin bottom-left; bit x of row word y (game.py:162-167, layout.py:108-112).
 *   - actions / directions: 0 North, 1 East, 2 South, 3 West, 4 Stop (gymPacMan.py:66-89).
 *   - agents 0,2 are red and start on the left half, agents 1,3 are blue (capture.py:316-319,
 *     gymPacMan.py:150,185,210); pmx_create rejects layouts where that does not hold.
 */
#ifndef PMX_H
#define PMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMX_VERSION 1
#define PMX_MAX_DIM 32      /* width and height <= 32: one uint32 per board row */
#define PMX_MAX_CAPSULES 4

enum {
    PMX_OK = 0,
    PMX_ERR_INVALID = -1,       /* bad argument / malformed layout */
    PMX_ERR_UNSUPPORTED = -2,   /* valid request this build does not implement */
    PMX_ERR_HIP = -3,           /* a HIP runtime call failed (message has the HIP error string) */
    PMX_ERR_NOMEM = -4
};

enum { PMX_OBS_F32 = 0, PMX_OBS_BF16 = 1, PMX_OBS_U8 = 2 };

/* Action code for an in-kernel randomTeam opponent (agents/randomTeam.py:90-100: random.choice(legal actions)):
 * the env itself picks uniformly among the agent's legal actions ON THE MID-TICK STATE, in the reference's list order
 * N,S,E,W,Stop, with a counter-based generator keyed by (config seed, env index, tick counter, agent).  The draw is
 * distribution-equivalent to the reference's (which uses Python's global Mersenne Twister) and is reproduced exactly
 * by the test oracle. */
#define PMX_ACTION_RANDOM_LEGAL (-2)
/* In-kernel baselineTeam opponents (agents/baselineTeam.py:65-187): the env scores the successor of every legal action of
 * the agent on the mid-tick state with the reference's reflex features and weights (offensive: -100 * food left - maze
 * distance to the nearest pellet; defensive: invaders, on-defence, invader distance, stop, reverse) and plays one of the
 * best actions (tie-break by the counter-based generator instead of random.choice); with no food left the agent walks home.
 * Only handles created with pmx_config.enable_bots understand these codes (the layouts' maze-distance matrices then stay
 * resident on the device, at most 2 GiB); elsewhere they act as Stop. */
#define PMX_ACTION_BASELINE_OFFENSE (-3)
#define PMX_ACTION_BASELINE_DEFENSE (-4)
/* In-kernel approxQTeam opponents (agents/approxQTeam.py), understood like the two codes above (enable_bots handles, mid-tick
 * state, any of the four agents; elsewhere Stop).
 * OFFENSE (ApproxQLearningOffense, :49-110, :194-292, TRAINING = False): with at most two pellets left to eat the agent walks
 * home exactly as the baseline bots do (no draw).  Otherwise Q(s, a) of every legal action is summed in float64, every product
 * and sum rounded on its own, in the order of the reference's feature dictionary:
 *     q = 0;  q += (1.0 / 10.0) * w_bias;  q += (g / 10.0) * w_ghosts;  if (g == 0 && the next cell holds a pellet the agent
 *     may eat) q += (1.0 / 10.0) * w_eats;  if (such a pellet is reachable) q += ((d / (width * height)) / 10.0) * w_closest
 * with the team file's four weights, next cell = the agent's cell plus the action vector, g = opponents that are not Pacman on
 * that cell or on one of its four neighbours, d = maze distance from the next cell to the nearest such pellet.  The best set
 * holds the actions whose q equals the maximum.  Three draws of the counter-based generator
 *     h(salt) = lowbias32(seed ^ env * 0x9E3779B1 ^ ticks * 0x85EBCA77 ^ agent * 0xC2B2AE3D ^ salt):
 *   explore iff h(0xA511E9B3) < 0x1999999A (= ceil(2^32 / 10), epsilon 0.1);
 *   when exploring, the action PMX_ACTION_RANDOM_LEGAL would play: the floor(h(0) * n / 2^32)-th of the n legal actions;
 *   otherwise the floor(h(0x5bd1e995) * m / 2^32)-th of the m best actions, the draw the baseline bots make
 * (lists in the order N, S, E, W, Stop).  Distribution-equivalent to util.flipCoin(0.1) + random.choice.
 * DEFENSE (DefensiveReflexAgent, :299-406): PMX_ACTION_BASELINE_DEFENSE, except that it walks home with at most two pellets
 * left (:324) where baselineTeam waits for none. */
#define PMX_ACTION_APPROXQ_OFFENSE (-5)
#define PMX_ACTION_APPROXQ_DEFENSE (-6)
/* Fog-bound bots (pmx_set_bot_sight below).  The reference's bots are written for the contest's observation: under
 * GameState.makeObservation (capture.py:268-292) getPosition() of a far enemy is None and the team files filter on it.  With a
 * bot sight set, bot agent I deciding on the mid-tick state e has mate M = (I + 2) % 4 and enemies O = (I + 1) % 4, (I + 3) % 4;
 *     seen(O) = min(manhattan(P[O], P[I]), manhattan(P[O], P[M])) <= sight_range,
 * all positions from e and never from a successor (the reference decides visibility once, in makeObservation; a hidden enemy
 * stays hidden in every successor generated from that observation).  Per action code:
 *     PMX_ACTION_BASELINE_DEFENSE, PMX_ACTION_APPROXQ_DEFENSE   an enemy counts as an invader of successor t (the -1000 and the
 *         distance term) iff t.pac[O] && seen(O)     (agents/baselineTeam.py:174, agents/approxQTeam.py:394)
 *     PMX_ACTION_APPROXQ_OFFENSE   g counts O iff !e.pac[O] && seen(O) and O is within one step of the next cell; eats follows
 *         g as before     (agents/approxQTeam.py:230)
 *     PMX_ACTION_BASELINE_OFFENSE, the walk home, PMX_ACTION_RANDOM_LEGAL and every draw (salts, order, count): unchanged.
 * The successors are the full state's.  A one-move successor can collide only with an enemy on the cell the mover reaches;
 * that enemy is at Manhattan distance at most 1 from P[I] before the move, hence seen for every sight_range >= 1, so the
 * transition needs no checkDeath skip (capture.py:681, :707).  That is why the range is 1 .. PMX_SIGHT_RANGE_MAX and 0 is
 * refused.  pmx_bot_query on such a handle also reports flag bit 2 = seen(the lower-index enemy), bit 3 = seen(the higher-index
 * enemy) for the codes -3 .. -6. */
#define PMX_BOT_SIGHT_OFF (-1)

typedef struct pmx_env pmx_env;

/* What gymPacMan_parallel_env.__init__ takes (gymPacMan.py:15) plus the batch size.  The .lay text is parsed
 * by the host language (layout.py:95-130); rows arrive bottom-up as bit masks. */
typedef struct {
    int32_t width, height;
    const uint32_t *wall_rows;   /* [height] '%' cells */
    const uint32_t *food_rows;   /* [height] '.' cells */
    const uint32_t *cap_rows;    /* [height] 'o' cells (at most PMX_MAX_CAPSULES bits) */
    const int8_t *starts;        /* [4][2] (x, y) of layout digits 1..4 = agents 0..3 (layout.py:113-114,128-129) */
    int32_t n_envs;              /* independent games advanced in lock-step */
    int32_t length;              /* `length` (gymPacMan.py:55): an episode lasts length+1 ticks (gymPacMan.py:268) */
    int32_t legal_reward;        /* reward_forLegalAction (gymPacMan.py:254-257) */
    int32_t defence_reward;      /* defenceReward (gymPacMan.py:238-242) */
    int32_t auto_reset;          /* 1: an env that terminates is reset inside the step, the way the reference's
                                    caller does right after a done (pacman_mappo_resnet.py:528-538); the
                                    observations/legal masks returned for it are those of the fresh game */
    int32_t obs_dtype;           /* PMX_OBS_*: element type of the observation planes (reference: float32) */
    int32_t obs_agents;          /* bit i set = emit agent i's observation; 0 means all four (0xF) */
    int32_t device;              /* HIP device ordinal */
    uint32_t seed;               /* key of the PMX_ACTION_RANDOM_LEGAL generator */
    int32_t n_layouts;           /* 0 or 1: every env plays the one layout above.  L > 1: wall_rows / food_rows / cap_rows
                                    hold [L][height] rows and starts [L][4][2]; all layouts share width x height; an env
                                    keeps the layout it is given unless redraw_layouts is set (below) */
    const int32_t *layout_index; /* [n_envs] host array: layout of each env (required when n_layouts > 1) */
    int32_t enable_bots;         /* 1: keep every layout's maze-distance matrix on the device and use the tick kernel variant
                                    that understands PMX_ACTION_BASELINE_* (it is a few microseconds per tick slower) */
    int32_t redraw_layouts;      /* 1 (needs n_layouts > 1): random_layout=True of the reference (gymPacMan.py:98-100 draws a new
                                    maze at every reset()): whenever an env is reset -- by pmx_reset or by the auto-reset inside
                                    pmx_step -- it moves to layout floor(u * n_layouts) of the pool, u from the counter-based
                                    generator keyed by (seed, env index, the env's tick counter); the layouts are the pool the
                                    host generated (maze_generator.py), layout_index gives the initial assignment.  The draw is
                                    distribution-equivalent to the reference's (which reseeds Python's global generator per maze)
                                    and is reproduced exactly by the test oracle. */
} pmx_config;

/* Outputs of one tick = what gymPacMan.step returns (gymPacMan.py:191-193), batched.  Any pointer may be
 * NULL to skip that output. */
typedef struct {
    void *obs_dev;               /* [n_envs][n_emit][8][H][W] obs_dtype; n_emit = popcount(obs_agents), agents in
                                    increasing index order.  Agent i's planes are encoded right after agent i's own
                                    sub-step (gymPacMan.py:166-167) */
    double *reward_dev;          /* [n_envs][2] team reward (red, blue) as float64, summed in the reference's order */
    uint8_t *done_dev;           /* [n_envs] terminations (gymPacMan.py:261-270) */
    uint8_t *legal_dev;          /* [n_envs][4] bit a = action a legal in the state the caller acts on next */
    int32_t *score_change_dev;   /* [n_envs] info['score_change'] */
    int32_t *score_dev;          /* [n_envs] game.state.data.score after the tick, BEFORE any auto-reset
                                    (pacman_mappo_resnet.py:529 reads it at a done) */
    uint32_t *agent_dev;         /* [n_envs][4] x | y << 8 | numCarrying << 16 of each agent right after its OWN sub-step,
                                    before any auto-reset: the content of observation plane 1 in compact form, which
                                    is all that get_agent_state / compute_heuristic_shaping read
                                    (pacman_mappo_resnet.py:241-264) */
} pmx_step_out;

/* Dynamic part of one game = the fields of capture.GameState / game.AgentState that the path reads
 * (game.py:120-131,374-396).  Used by pmx_get_state / pmx_set_state, fixtures and the GameState facade. */
typedef struct {
    int8_t pos[4][2];
    int8_t dir[4];               /* configuration.direction */
    uint8_t pac[4];              /* isPacman */
    uint8_t scared[4];           /* scaredTimer */
    uint16_t carry[4];           /* numCarrying */
    uint16_t ret[4];             /* numReturned */
    uint32_t food[PMX_MAX_DIM];
    uint32_t caps[PMX_MAX_DIM];
    int32_t score;
    int32_t steps;               /* gymPacMan_parallel_env.steps */
    uint32_t ticks;              /* ticks since pmx_create (never reset): counter of the random-legal generator */
} pmx_state;

int pmx_version(void);
const char *pmx_last_error(void);

/* gymPacMan_parallel_env.__init__ (gymPacMan.py:15-89) + CaptureRules.newGame (capture.py:369-382): validates the
 * layout, allocates device state for n_envs games and puts every game in its initial state. */
int pmx_create(const pmx_config *cfg, pmx_env **out);
int pmx_destroy(pmx_env *env);

/* shape helpers for the binding */
int pmx_obs_shape(const pmx_env *env, int32_t *n_emit, int32_t *height, int32_t *width, int32_t *elem_bytes);

/* gymPacMan_parallel_env.reset (gymPacMan.py:92-141).  mask_dev: [n_envs] non-zero = reset that env; NULL = all.
 * out (may be NULL): obs_dev / legal_dev are filled for ALL envs from their current state (the four agents see
 * the same state, gymPacMan.py:135-137); the other members are ignored. */
int pmx_reset(pmx_env *env, const uint8_t *mask_dev, const pmx_step_out *out, void *stream);

/* gymPacMan_parallel_env.step with self_play=True (gymPacMan.py:143-193): actions_dev [n_envs][4] int8, one
 * requested action per agent; an illegal or out-of-range action becomes Stop (capture.py:473-474). */
int pmx_step(pmx_env *env, const int8_t *actions_dev, const pmx_step_out *out, void *stream);

/* One agent's sub-step of the same tick (the body of the loop gymPacMan.py:149-169), so that host-side
 * CaptureAgent bots can choose on the mid-tick state (gymPacMan.py:157).  Call with agent = 0,1,2,3 in this
 * order; actions_dev [n_envs] int8.  out->obs_dev, if set, receives [n_envs][8][H][W] for this agent.  The
 * call with agent == 3 closes the tick: reward/done/legal/score_change/score are written then (and only then),
 * and auto-reset, if configured, is applied. */
int pmx_step_agent(pmx_env *env, int agent, const int8_t *actions_dev, const pmx_step_out *out, void *stream);

/* GameState.generateSuccessor (capture.py:107-123) applied in place to every env: agent `agent` takes actions_dev[env]
 * (int8 [n_envs]).  No reward, no tick bookkeeping, no termination test: this is the query CaptureAgent bots make on
 * hypothetical states (agents/baselineTeam.py:94-104), normally on a small scratch handle loaded with pmx_set_state.
 * score_change_dev (may be NULL) receives data.scoreChange of each successor. */
int pmx_successor(pmx_env *env, int agent, const int8_t *actions_dev, int32_t *score_change_dev, void *stream);

/* Ask an in-kernel bot for its move: for agent `agent` of every env, on the CURRENT state and without changing it, what bot
 * `code` (PMX_ACTION_RANDOM_LEGAL .. PMX_ACTION_APPROXQ_DEFENSE) computes and what it would play if
 * pmx_step_agent(env, agent, code) were called now (same tick counter, same draws; the tick and this query run the same device
 * functions).  values_dev [n_envs][5] float64 indexed by action code: the q above for PMX_ACTION_APPROXQ_OFFENSE, the integer
 * feature sum as a double for the three reflex codes, 0.0 for PMX_ACTION_RANDOM_LEGAL; NaN for illegal actions.  action_dev
 * [n_envs] int8.  flags_dev [n_envs]: bit 0 = the agent walks home, bit 1 = it explored.  Any of the three may be NULL.
 * PMX_ERR_UNSUPPORTED on a handle without enable_bots (except PMX_ACTION_RANDOM_LEGAL), PMX_ERR_INVALID for a bad agent or
 * code. */
int pmx_bot_query(pmx_env *env, int agent, int code, double *values_dev, int8_t *action_dev, uint8_t *flags_dev, void *stream);

/* Bind the in-kernel bots to the contest's sight rule (the table at PMX_BOT_SIGHT_OFF above).  A host-side field of the
 * handle, no launch: it applies to every pmx_step, pmx_step_agent and pmx_bot_query enqueued after the call, which then run
 * separate instantiations of their kernels.  PMX_BOT_SIGHT_OFF, the default, restores the kernels of a handle never set.
 * sight_range is PMX_BOT_SIGHT_OFF or 1 .. PMX_SIGHT_RANGE_MAX (from 62 on nothing is hidden); PMX_ERR_INVALID for a NULL
 * handle or any other value, PMX_ERR_UNSUPPORTED for a value other than PMX_BOT_SIGHT_OFF on a handle without enable_bots. */
int pmx_set_bot_sight(pmx_env *env, int32_t sight_range);

/* Observation planes / legal masks of the CURRENT state for all emitted agents (gymPacMan.get_Observation,
 * gymPacMan.py:195-229; GameState.getLegalActions, capture.py:101-105). */
int pmx_observe(pmx_env *env, void *obs_dev, uint8_t *legal_dev, void *stream);

/* What the MAPPO rollout does with every tick's observations (pacman_mappo_resnet.py:462-469), straight from the env: the two
 * observations of one team -- agents (0, 2) when team_red, else (1, 3); agent i's planes from the state right after its own
 * sub-step, exactly as pmx_step emits them -- written as team_obs_dev [n_envs][2][8][H][W] of the handle's obs_dtype and
 * CANONICALISED for a red team (canonicalize_obs :215-229: x flipped, planes 2 <-> 3 and 6 <-> 7 swapped), plus, if merged_dev
 * is not NULL, merge_obs_for_critic of the two (:267-274) as [n_envs][8][H][W].  Valid after pmx_step (tick observations) and
 * after pmx_reset / pmx_set_state (all agents see the current state). */
int pmx_emit_team_obs(pmx_env *env, int team_red, void *team_obs_dev, void *merged_dev, void *stream);

/* pmx_emit_team_obs with the learners' colour chosen PER ENV, for a rollout whose envs play different pairings at once (the
 * reference draws one opponent and one side per rollout of its single env, pacman_mappo_resnet.py:396-438; the frames are
 * those of :215-229 and :267-274).  team_red_dev [n_envs] uint8, non-zero = this env's learners are red.  Rows are written for
 * the envs first .. first + count - 1 only, output row j for env first + j: team_obs_dev [count][2][8][H][W], merged_dev
 * [count][8][H][W] or NULL.  Row e - first is byte for byte row e of pmx_emit_team_obs(env, team_red_dev[e] != 0, ...).
 * count == 0 launches nothing; PMX_ERR_INVALID for a range outside the handle's envs. */
int pmx_emit_team_obs_mixed(pmx_env *env, const uint8_t *team_red_dev, int32_t first, int32_t count, void *team_obs_dev,
                            void *merged_dev, void *stream);

/* The contest's sight rule on the learners' planes (GameState.makeObservation, capture.py:268-292, which gymPacMan's
 * get_Observation never applies).  The two calls above with one difference: in a learner's plane 5 the cell of enemy e is 0
 * unless min over the two team agents m of |x_e - x_m| + |y_e - y_m| <= sight_range, all positions taken from the snapshot
 * that learner's planes are encoded from.  The rule is the team's (an enemy next to either learner shows in both), and the two
 * learners read different snapshots, so one enemy can show in one slot and not in the other.  The merged slot is the
 * full-information critic input: byte for byte that of the call without fog.  sight_range 0 .. PMX_SIGHT_RANGE_MAX, anything
 * else is PMX_ERR_INVALID and launches nothing; from 62 on (the longest distance on a 32 x 32 board) nothing is hidden. */
#define PMX_SIGHT_RANGE 5       /* capture.py:69 */
#define PMX_SIGHT_RANGE_MAX 64
int pmx_emit_team_obs_fog(pmx_env *env, int team_red, int32_t sight_range, void *team_obs_dev, void *merged_dev, void *stream);
int pmx_emit_team_obs_mixed_fog(pmx_env *env, const uint8_t *team_red_dev, int32_t first, int32_t count, int32_t sight_range,
                                void *team_obs_dev, void *merged_dev, void *stream);

/* ---- Belief sets: what a team can know about the enemies the sight rule hides ------------------------------------------------
 * Besides the sight rule the contest gives a team a noisy distance to every agent at every turn (capture.py:67-78 SONAR_NOISE_RANGE
 * = 13, :210-224 noisyDistance, :268-275 makeObservation).  The tracker below turns those readings, the sight rule and the rules
 * of motion into, per learner slot and hidden enemy, the SET of cells the enemy can be on -- possibilistic, not weighted: a cell is
 * in or out -- and the belief emission writes the sets into plane 5, the plane that holds the enemies, with values 0 or 1.  All of
 * it is integer and exact.
 *
 * Team and enemies.  For a team of colour `red`: first = red ? 0 : 1, second = first + 2.  Enemy k (0 or 1) is agent
 * e_k = (1 - first) + 2 k.  Slot j (0 or 1) belongs to learner a_j = first + 2 j and is read from the snapshot that learner's
 * planes are encoded from, the snapshots pmx_emit_team_obs reads; P[i] is agent i's cell in it.
 *
 * Belief buffer (caller-owned): uint32_t belief[rows][2 slots][2 enemies][32].  Bit x of word y = the enemy can be on cell (x, y),
 * raw coordinates (not flipped); words y >= H are 0.  512 contiguous bytes per env.
 *
 * Sonar reading of learner a_j for enemy e_k: r = manhattan(P[a_j], P[e_k]) + n, n = (int)(((uint64_t)h * 13) >> 32) - 6 in
 * -6 .. 6, h = h(PMX_SALT_SONAR) the counter-based generator documented at PMX_ACTION_APPROXQ_OFFENSE with `agent` =
 * 4 a_j + e_k and `ticks` = the env's ticks word at the time of the call (the value pmx_get_state returns).  Distribution-
 * equivalent to noisyDistance; r may be negative, as in the reference.
 *
 * pmx_belief_update, once after each pmx_step, for the envs first .. first + count - 1 (belief / sonar row env - first; colour
 * team_red_dev[env] != 0, or the uniform team_red when team_red_dev is NULL).  For slot j = 0, then j = 1, and both enemies k:
 *   1. starting set  S = the previous call's slot-1 set when j == 0, the slot-0 set just computed when j == 1;
 *   2. motion        if e_k == (a_j + 3) % 4 -- the enemy whose sub-step lies between the two snapshots --
 *                    S = (S | S << 1 | S >> 1 | row above | row below) & open cells  (Stop is a move; an extra dilation is never unsound);
 *   3. respawn       S |= bit(start cell of e_k): every death returns an agent to its start, whoever's move caused it, so the
 *                    rule is sound for every sight_range;
 *   4. sight         seen = min over m in {first, second} of manhattan(P[e_k], P[m]) <= sight_range (the fog kernels' rule).
 *                    Seen: S = bit(P[e_k]).  Otherwise every cell within sight_range of P[first] or P[second] leaves S, and so
 *                    does every cell c with |manhattan(P[a_j], c) - r| > 6;
 *   5. store         belief[row][j][k] = S; sonar_dev[row][j][k] = r (int8 [count][2][2], may be NULL).
 * reset_dev (uint8 [n_envs], may be NULL; pass `done` of the last step under auto_reset): where reset_dev[env] != 0 the steps are
 * skipped, both slots of both enemies become the enemy's start cell in the env's CURRENT layout (redraw_layouts) and the four
 * readings are 0.  PMX_ERR_INVALID for a range outside the handle's envs or a sight_range outside 0 .. PMX_SIGHT_RANGE_MAX;
 * count == 0 launches nothing.  An open profile (pmx_profile_begin) records the launch with the rule launches.
 *
 * pmx_belief_init takes no colour, so a buffer can be set up before the learners' colour is drawn.  kind 0 (valid after pmx_reset):
 * the sets of enemy k, in both slots, hold the start cells of agents 2 k and 2 k + 1 -- enemy k of a blue and of a red team -- which
 * is sound for either colour; the updates' sight and sonar rules narrow it.  kind 1 (valid after pmx_set_state, or
 * when the learners' colour changes): every set holds every open cell.  Any other kind is PMX_ERR_INVALID. */
#define PMX_SALT_SONAR 0x534F4E41u
int pmx_belief_update(pmx_env *env, int team_red, const uint8_t *team_red_dev, int32_t first, int32_t count, int32_t sight_range,
                      const uint8_t *reset_dev, uint32_t *belief_dev, int8_t *sonar_dev, void *stream);
int pmx_belief_init(pmx_env *env, int32_t first, int32_t count, int32_t kind, uint32_t *belief_dev, void *stream);
/* pmx_emit_team_obs / pmx_emit_team_obs_mixed with one difference: learner slot j's plane 5 is belief[row][j][0] | belief[row][j][1]
 * (row = the output row), x-flipped for red like every other plane, in place of the enemies' own bits.  A seen enemy is a one-cell
 * set, so no sight test runs here.  Every other plane and the whole merged slot -- the full-information critic input -- are byte
 * for byte those of the plain call.  The buffer is read, never written. */
int pmx_emit_team_obs_belief(pmx_env *env, int team_red, const uint32_t *belief_dev, void *team_obs_dev, void *merged_dev, void *stream);
int pmx_emit_team_obs_mixed_belief(pmx_env *env, const uint8_t *team_red_dev, int32_t first, int32_t count, const uint32_t *belief_dev,
                                   void *team_obs_dev, void *merged_dev, void *stream);

/* ---- Belief weights: an exact Bayes filter that refines the sets ----------------------------------------------------------------
 * A set cannot say that one cell is a hundred times less likely than another.  The weighted tracker keeps, beside every set, an
 * integer weight per cell: the contest's standard exact inference with a uniform random walk over the legal moves (Stop included)
 * as the motion model, a small respawn prior on the start cell, the sight rule, and the sonar, whose likelihood is flat over its 13
 * values and so only cuts the annulus the set rule already cuts.  All integer and exact; the support of the weights IS the set.
 *
 * Buffers (caller-owned), HW = H * W of the handle, cell c = y * W + x in raw (not flipped) coordinates:
 *   belief   uint32_t [rows][2][2][32]          the sets, advanced by the table of "Belief sets" unchanged
 *   weights  uint16_t [rows][2 slots][2 enemies][HW]
 *   levels   uint8_t  [rows][2 slots][HW]       what the weighted emission shows, 0 .. PMX_BELIEF_LEVELS
 * R[d] = floor(65536 / d): 65536, 32768, 21845, 16384, 13107 for d = 1 .. 5.  deg(n) = 1 + the number of open 4-neighbours of cell
 * n, the count of legal actions there, Stop included.
 *
 * pmx_belief_weights_update REPLACES pmx_belief_update (same arguments plus the two buffers; it is not run in addition): it draws
 * the same readings with the same key, salt and tick word and applies the same five steps to the sets, so belief and sonar_dev come
 * out bit for bit as pmx_belief_update leaves them.  Beside them, for slot j = 0, then j = 1, and both enemies k:
 *   1. start      q = the previous call's slot-1 weights when j == 0, the slot-0 weights just computed when j == 1;
 *   2. motion     for the enemy that moved (the set rule's condition, e_k == (a_j + 3) % 4):
 *                 t[c] = sum over n in {c} + N4(c), n open, of (q[n] * R[deg(n)]) >> 16 for open c, 0 on walls, in uint32;
 *                 for the other enemy t = q;
 *   3. respawn    t[start cell of e_k] += 1 + (T >> PMX_BELIEF_RESPAWN_SHIFT), T = sum of t: about 1/64 of the mass per tick over
 *                 the two slots.  A modelling constant, not a measured one;
 *   4. sight and sonar   S' = the set this step produces (step 4 of the set table).  Enemy seen: q' = 65535 on its cell, 0
 *                 elsewhere, and step 5 is skipped.  Hidden: u[c] = max(t[c], 1) for c in S', 0 elsewhere; the floor of 1 makes
 *                 support(q') == S' hold exactly whatever the rounding did;
 *   5. normalise  by a shift, no division: m = max u, b = 32 - clz(m).  b > 16: q'[c] = max(u[c] >> (b - 16), 1) on S';
 *                 otherwise q'[c] = u[c] << (16 - b); S' empty: q' = 0.  Hence 32768 <= max q' <= 65535 for a hidden enemy;
 *   6. store      weights[row][j][k] = q';  levels[row][j][c] = max over k of (q'_k[c] == 0 ? 0 : 1 + (q'_k[c] >> 12)), 0 .. 16:
 *                 a seen enemy's cell is 16, a hidden enemy's mode cell 9 .. 16.
 * Bounds: q <= 65535 and R <= 65536, so a product is below 2^32; t[c] <= 5 * 65535; T <= 1024 * 5 * 65535 < 2^32;
 * u <= 5 * 65535 + 1 + (T >> 7) < 2^22.
 * reset_dev[env] != 0: as for the sets -- both slots of both enemies become 65535 on the enemy's start cell in the env's current
 * layout, the levels 16 there, the readings 0.  Errors as pmx_belief_update, and PMX_ERR_INVALID for a NULL weights_dev or
 * levels_dev; count == 0 launches nothing.
 *
 * pmx_belief_weights_init: belief as pmx_belief_init writes it; weights 65535 on the cells of each set (kind 0: the start cells,
 * kind 1: every open cell) in both slots, 0 elsewhere; levels 16 on the union of the two enemies' sets, so an emission straight
 * after it is valid. */
#define PMX_BELIEF_RESPAWN_SHIFT 7
#define PMX_BELIEF_LEVELS 16
int pmx_belief_weights_update(pmx_env *env, int team_red, const uint8_t *team_red_dev, int32_t first, int32_t count, int32_t sight_range,
                              const uint8_t *reset_dev, uint32_t *belief_dev, int8_t *sonar_dev, uint16_t *weights_dev, uint8_t *levels_dev,
                              void *stream);
int pmx_belief_weights_init(pmx_env *env, int32_t first, int32_t count, int32_t kind, uint32_t *belief_dev, uint16_t *weights_dev,
                            uint8_t *levels_dev, void *stream);
/* pmx_emit_team_obs_belief / _mixed_belief with levels_dev in place of belief_dev and one difference: learner slot j's plane 5 is
 * levels[row][j] (x-flipped for red like every other plane) as a NUMBER in the output's element type -- the byte itself in uint8
 * planes, the exactly converted integer in bfloat16 and float32.  Every other plane and the whole merged slot are byte for byte
 * the plain call's.  The buffer is read, never written. */
int pmx_emit_team_obs_weighted(pmx_env *env, int team_red, const uint8_t *levels_dev, void *team_obs_dev, void *merged_dev, void *stream);
int pmx_emit_team_obs_mixed_weighted(pmx_env *env, const uint8_t *team_red_dev, int32_t first, int32_t count, const uint8_t *levels_dev,
                                     void *team_obs_dev, void *merged_dev, void *stream);

/* ---- Belief evidence: the public facts the observation leaves on a hidden enemy ---------------------------------------------------
 * makeObservation (capture.py:268-292) blanks only the `configuration` of a hidden enemy: both food grids, every agent's isPacman
 * and the team's own positions stay in what every contest agent gets.  The evidence forms of the two updates use them.  Opt-in:
 * pmx_belief_update / pmx_belief_weights_update are unchanged, and these calls REPLACE them (same arguments plus `rules` and the
 * evidence buffer).  All integer and exact.
 *
 *   rule (bit of `rules`)        fact                                          effect on enemy e_k's set in slot j
 *   PMX_EVIDENCE_SIDE     1      isPacman of a hidden enemy (capture.py:492)   only the columns of the half it is on stay
 *   PMX_EVIDENCE_FOOD     2      a pellet left the defended half               the mover stands where the pellet was
 *   PMX_EVIDENCE_CONTACT  4      a death is a collision with a team agent      the start cell joins only a set that touches one
 *
 * Evidence buffer (caller-owned): uint32_t evidence[rows][PMX_EVIDENCE_WORDS], 144 bytes per env, row = env - first.  Words 0 .. 31:
 * the food row words of the slot-1 snapshot at the last update (both halves; rows >= H are 0).  Word 32 / 33: P[first] / P[second]
 * in that snapshot as x | y << 8.  Word 34: 1 if words 0 .. 33 are valid, else 0.  Word 35: 0.  pmx_belief_evidence_init zeroes
 * the rows (valid = 0); call it wherever pmx_belief_init / pmx_belief_weights_init is called on those rows.
 *
 * Notation as in "Belief sets", and: half, lo_mask (columns x < half), hi_mask from the layout; mine = lo_mask for a red team (it
 * defends x < half), hi_mask for a blue one.  The previous snapshot of slot 1 is slot 0's snapshot of this call; that of slot 0 is
 * the evidence row, and when word 34 is 0 slot 0 has none.  F_prev, F: the food rows of the previous snapshot and of slot j's;
 * P_prev[first], P_prev[second]: the team's two cells in the previous snapshot.
 *
 * The steps of the set table that change, per slot j and enemy k:
 *   2a. food     (rules & 2, a previous snapshot exists, e_k is the enemy that moved)  E = F_prev & ~F & mine over all rows.  If E
 *                has exactly one bit c, manhattan(c, P_prev[a_j]) > 1 and manhattan(c, start cell of a_j) > 1: after the dilation,
 *                S &= E.  Sound because only a mover standing on a pellet removes it (capture.py:514-560) and the window holds
 *                exactly two movers, e_k and then a_j; a returning agent can eat food on its own half (quirk Q1, SURVEY.md appendix
 *                A), so a_j is excluded by where it can have been: one step from its previous cell, or from its start if it was
 *                killed in between.  E with more than one bit cannot arise from play; the rule is skipped then (a hand-set state).
 *   3. respawn   without rules & 4, or without a previous snapshot: S |= start bit, as before.  Otherwise K = the cells within
 *                Manhattan distance 1 of P_prev[first], P_prev[second] and the start cells of first and second, and S |= start bit
 *                only if S & K is not empty: every death is a same-cell collision with one of the team's agents (capture.py:
 *                670-728); the stationary agent is on its previous cell, the learner one step from its previous cell or its start.
 *   4. side      (rules & 1, hidden enemies only, after the sight and sonar cuts)  S &= ((x of P[e_k] < half) == red) ? mine : the
 *                other half's columns.  The flag is taken from the position, not from bit 24 of the agent word, so that a state
 *                set from outside with an inconsistent flag cannot make the set unsound.
 *   5. store     after slot 1 the evidence row is written from slot 1's snapshot with valid = 1.  Reset rows (reset_dev[env] != 0)
 *                get sets and readings as before; their evidence row is written from the current slot-1 snapshot too, which under
 *                auto_reset holds the fresh game, with valid = 1.
 * rules == 0 leaves belief and sonar_dev bit for bit as pmx_belief_update leaves them; the evidence row is still maintained.
 * pmx_belief_weights_update_evidence applies this set rule and then the table of "Belief weights" unchanged with S' this set; the
 * mass its step 3 puts on a start cell outside S' is dropped by its step 4.
 * Errors as the parent call, and PMX_ERR_INVALID for rules outside 0 .. 7 or a NULL evidence_dev. */
#define PMX_EVIDENCE_SIDE    1
#define PMX_EVIDENCE_FOOD    2
#define PMX_EVIDENCE_CONTACT 4
#define PMX_EVIDENCE_WORDS   36
int pmx_belief_evidence_init(pmx_env *env, int32_t first, int32_t count, uint32_t *evidence_dev, void *stream);
int pmx_belief_update_evidence(pmx_env *env, int team_red, const uint8_t *team_red_dev, int32_t first, int32_t count, int32_t sight_range,
                               int32_t rules, const uint8_t *reset_dev, uint32_t *belief_dev, int8_t *sonar_dev, uint32_t *evidence_dev,
                               void *stream);
int pmx_belief_weights_update_evidence(pmx_env *env, int team_red, const uint8_t *team_red_dev, int32_t first, int32_t count,
                                       int32_t sight_range, int32_t rules, const uint8_t *reset_dev, uint32_t *belief_dev, int8_t *sonar_dev,
                                       uint16_t *weights_dev, uint8_t *levels_dev, uint32_t *evidence_dev, void *stream);

/* ---- Episode statistics (opt-in, no reference counterpart): an exact per-episode event record for every env ------------------
 * The env reports rewards, done and the score; who ate, who died carrying what and who caught whom is in none of them.  The
 * sub-step snapshots a tick leaves (the ones the observation and belief kernels read) hold all of it, and this kernel counts it.
 * stats_dev is caller-owned: int32 [PMX_STATS_WORDS][count], WORD-MAJOR -- word w of row r = env - first is stats_dev[w * count + r],
 * the state's own structure-of-arrays order, so the lane-per-env kernel reads and writes it coalesced.  Words:
 *   8 i + c     counter c (PMX_STAT_*) of agent i
 *   32 TICKS    33 SCORE (data.score after the last counted tick, signed)    34 DONE    35 0
 *   36..39 / 40..43   agent words A / B of the state after the last counted tick (x | y << 8 | dir << 16 | isPacman << 24 and
 *                     scaredTimer | numCarrying << 8 | numReturned << 20)
 *   44, 45      its two capsule words (four 16-bit slots x | y << 8, 0xFFFF = empty)        46, 47   0
 * pmx_episode_stats_init, after pmx_reset or pmx_set_state and before the first step: zeroes the counters, TICKS, DONE and words 35,
 * 46, 47 and sets SCORE and words 36..45 from the current state.
 * pmx_episode_stats_update, once after each pmx_step: a row whose DONE word is not 0 is left untouched, every word of it.  Otherwise
 * the four sub-step transitions X -> Y of the tick are walked with mover m = 0, 1, 2, 3 over the states: words 36..45, snapshot 0,
 * snapshot 1, snapshot 2, current state.  pos = (x, y), dist = Manhattan distance, every field from the agent and capsule words:
 *   death of a non-mover i != m   pos_Y[i] != pos_X[i], or scared_X[i] > 0 && scared_Y[i] == 0, or carry_Y[i] < carry_X[i]  (only the
 *                                 mover moves, only the mover's timer ticks, and only a death empties another agent's carry)
 *   death of the mover            dist(pos_Y[m], pos_X[m]) > 1, or carry_Y[m] < carry_X[m] && ret_Y[m] == ret_X[m], or
 *                                 scared_X[m] >= 2 && scared_Y[m] == 0
 *   DEATHS[i]       += 1 per death of i
 *   LOST[i]         += carry_X[i] per death of i
 *   KILLS[m]        += number of non-movers that died
 *   EATEN[m]        += max(0, carry_Y[m] - carry_X[m])
 *   RETURNED[m]     += ret_Y[m] - ret_X[m]
 *   CAPSULES[m]     += occupied capsule slots of X minus those of Y
 *   PACMAN_STEPS[m] += isPacman_Y[m]
 *   STOPS[m]        += 1 if the mover did not die and pos_Y[m] == pos_X[m]  (illegal actions become Stop, capture.py:473-474)
 * After the four transitions TICKS += 1, SCORE = the state's score word, words 36..45 = the state's, DONE = 1 where done_dev[env]
 * != 0 (done_dev [n_envs] uint8, indexed by env, may be NULL: DONE is then never set).
 * Blind spot: a mover with carry == 0 and scared <= 1 that is sent to a start cell within one step of the cell it left is counted
 * as a move.  In the reference this can only be a scared ghost with one tick of fear left that steps onto an invader beside its
 * own start.  Non-movers have none: a Pacman never stands on its own start, and a ghost there that is not scared cannot be eaten.
 * A mover that eats a pellet and dies in the same move (capture.py applies the action before checkDeath) gets EATEN += 0 and LOST
 * += carry_X, so EATEN - RETURNED - LOST == numCarrying stays exact.
 * One lane per env, no LDS, no atomics, plain vector stores (csrc/pmx_stats.hip).  An open pmx_profile_begin records the update with
 * the rule launches, as the belief update's.
 * Errors: PMX_ERR_INVALID for a NULL handle or buffer, a range outside the handle, an unfinished pmx_step_agent tick and, for the
 * update, where the snapshots do not describe the last tick (nothing stepped since pmx_reset / pmx_set_state, or the tick was run
 * with pmx_step_agent or pmx_successor, which leave no snapshots); PMX_ERR_UNSUPPORTED on an auto_reset handle (a finished env's
 * snapshots and state are overwritten with the fresh game inside the tick, so its terminal tick cannot be read).  count == 0
 * launches nothing. */
#define PMX_STATS_WORDS 48
enum { PMX_STAT_EATEN, PMX_STAT_RETURNED, PMX_STAT_LOST, PMX_STAT_DEATHS, PMX_STAT_KILLS, PMX_STAT_CAPSULES, PMX_STAT_PACMAN_STEPS, PMX_STAT_STOPS };  /* 8 per agent */
int pmx_episode_stats_init(pmx_env *env, int32_t first, int32_t count, int32_t *stats_dev, void *stream);
int pmx_episode_stats_update(pmx_env *env, int32_t first, int32_t count, const uint8_t *done_dev, int32_t *stats_dev, void *stream);

/* ---- Game records (opt-in): a device log of every sub-step of chosen envs, for replay and text rendering -------------------------
 * The reference's users have capture.py --record / --replay and textDisplay; a game played on the device, bots deciding inside the
 * tick kernel, leaves only counters.  The sub-step snapshots hold everything a replay needs, and this kernel keeps them.
 * Both buffers are caller-owned int32, WORD-MAJOR with the row innermost like stats_dev; row r is env first + r:
 *   head_dev   [PMX_RECORD_HEAD_WORDS][count]   word w of row r = head_dev[w * count + r]
 *       0 LEN (ticks recorded)   1 DONE   2 OVERFLOW   3 LAYOUT (the row's layout index at init, 0 on a single-layout handle)   4..7  0
 *   frames_dev [1 + 4 * max_ticks][FW][count]   word w of frame f of row r = frames_dev[(f * FW + w) * count + r], FW = 12 + height
 *       (pmx_game_record_words).  Frame 0 is the state at init; frame 1 + 4 t + m the state after sub-step m of recorded tick t:
 *       snapshot m for m = 0, 1, 2 and the current state for m = 3.
 * One frame:
 *   0..3 / 4..7   agent words A / B, the encoding of stats words 36..43      8, 9   the two capsule words (stats words 44, 45)
 *   10            data.score after the sub-step, signed.  The snapshots carry no score word, and need none: only the mover's
 *                 returned pellets move the score (capture.py:495-511), so after sub-steps 0 .. 2 it is the previous frame's score
 *                 + (ret_Y[m] - ret_X[m]) for a red mover, - for a blue one; after sub-step 3 it is the state's own score word.
 *   11            EVENT (below)                                              12 .. 12 + height - 1   food rows, bit x of row y
 * EVENT of sub-step m, the transition X -> Y with X the previous frame (EVENT of frame 0 is 0):
 *   bits 0..2     the move that was made: 0 North, 1 East, 2 South, 3 West, 4 Stop (the env's action codes), 7 undetermined
 *   bit 3         the mover died
 *   bits 4..7     mask of the non-movers that died (bit 4 + i: agent i)
 *   bit 8         the mover ate a pellet (carry_Y[m] > carry_X[m])
 *   bit 9         a capsule was eaten (occupied capsule slots of X > those of Y)
 *   bits 10..21   ret_Y[m] - ret_X[m]
 * Deaths are decided by the table of "Episode statistics".  The move of a mover that did not die is the direction of pos_Y[m] -
 * pos_X[m], Stop where the two are equal (an illegal request became Stop, capture.py:473-474).  The move of a mover that died is
 * the unique d of the five for which pos_X[m] + d is the cell of an enemy in X (every death is a same-cell collision, capture.py:
 * 670-728); 7 where no d or more than one qualifies.
 * pmx_game_record_init, after pmx_reset or pmx_set_state and before the first step: zeroes the head but LAYOUT and writes frame 0.
 * pmx_game_record_update, once after each pmx_step: a row whose DONE or OVERFLOW word is not 0 is left untouched, every word of it.
 * A row with LEN == max_ticks (or a LEN outside 0 .. max_ticks) gets OVERFLOW = 1 and nothing else.  Any other row gets the four
 * frames 4 LEN + 1 .. 4 LEN + 4, LEN += 1, and DONE = 1 where done_dev[env] != 0 (done_dev [n_envs] uint8, indexed by env, may be
 * NULL: DONE is then never set).  X of sub-step 0 is read back from the log, frame 4 LEN.  max_ticks must be the value of init.
 * Blind spot: the stats kernel's own (a scared ghost with one tick of fear left that steps onto an invader beside its own start is
 * logged as a move, bit 3 clear), plus move code 7: a mover that died with two enemy cells, or none, within one step of the cell
 * it left.  The frames themselves are exact in either case.
 * One lane per env, no LDS, no atomics, plain vector stores (csrc/pmx_record.hip); no other kernel changes.  An open
 * pmx_profile_begin records the update with the rule launches, as the stats update's.
 * Errors: those of the stats calls (PMX_ERR_INVALID for a NULL handle or buffer, a range outside the handle, an unfinished
 * pmx_step_agent tick and, for the update, where the snapshots do not describe the last tick; PMX_ERR_UNSUPPORTED on an auto_reset
 * handle), and PMX_ERR_INVALID for max_ticks < 1.  count == 0 launches nothing. */
#define PMX_RECORD_HEAD_WORDS 8
enum { PMX_RECORD_LEN, PMX_RECORD_DONE, PMX_RECORD_OVERFLOW, PMX_RECORD_LAYOUT };
int pmx_game_record_words(const pmx_env *env, int32_t *frame_words);      /* FW = 12 + H */
int pmx_game_record_init(pmx_env *env, int32_t first, int32_t count, int32_t max_ticks, int32_t *head_dev, int32_t *frames_dev, void *stream);
int pmx_game_record_update(pmx_env *env, int32_t first, int32_t count, int32_t max_ticks, const uint8_t *done_dev, int32_t *head_dev,
                           int32_t *frames_dev, void *stream);

/* ---- Sight rule on the four-agent planes (opt-in): the contest's observation on pmx_step / pmx_step_agent / pmx_observe / pmx_reset
 * gymPacMan's get_Observation hands every agent the full state; the contest hands agent i GameState.makeObservation(i)
 * (capture.py:268-292): the state with the configuration of every far enemy blanked, and four noisy distances.  The two calls below
 * put both on the env's own surfaces; the team entry points above (pmx_emit_team_obs_fog, pmx_belief_update) are unchanged.
 *
 * pmx_set_obs_sight: a host-side field of the handle, no launch, like pmx_set_bot_sight.  PMX_OBS_SIGHT_OFF (the default) or
 * 0 .. PMX_SIGHT_RANGE_MAX; PMX_ERR_INVALID for a NULL handle or any other value.  While a range is set, every four-agent observation
 * the handle writes afterwards -- obs_dev of pmx_step, pmx_step_agent, pmx_observe and pmx_reset, for every obs_agents subset, element
 * type and per-env layout -- is under this rule, for agent i with mate m = i ^ 2 and enemies o (o ^ i odd):
 *
 *   what                         from                                                        reference
 *   P[0 .. 3]                    the snapshot agent i's planes are encoded from (after its     gymPacMan.py:166-167
 *                                own sub-step in pmx_step, the current state otherwise)
 *   seen(o)                      min(manhattan(P[o], P[i]), manhattan(P[o], P[m]))            capture.py:285-291
 *                                <= sight_range
 *   plane 5 of agent i           the cell of enemy o is set iff seen(o)                       capture.py:288-290 (configuration = None)
 *   planes 0 - 4, 6, 7           unchanged: walls, self, capsules, the mate, both food grids   capture.py:268-292 blanks nothing else
 *
 * This is the rule of pmx_emit_team_obs_fog applied to agent i's own block.  Every other plane byte and every other output of the
 * call (reward, done, legal, score change, score, agent words), the state and the snapshots are byte for byte what they are with the
 * rule off; from 62 on nothing is hidden.  With a range set pmx_step runs the rule launch followed by the sight form of the expansion
 * kernel: neither the one-launch tick nor the wall split is taken, pmx_last_step_fused reports 0 and an open profile records the
 * expansion as an expand launch.  uint8 planes of four agents take the wave per (env, agent) kernel.  After PMX_OBS_SIGHT_OFF the
 * handle takes exactly the paths of a handle never set.
 *
 * pmx_agent_distances: the contest's getAgentDistances() (capture.py:210-224 noisyDistance, :272-275) for every env.
 *   agent == -1       dist_dev int8 [n_envs][4][4], 16-byte aligned: r[a][i] = manhattan(P_a[a], P_a[i]) + n for every target i, a itself
 *                     and its mate included (as the reference), P_a from the source agent a's planes are encoded from: its snapshot
 *                     after a pmx_step, the current state otherwise -- what pmx_emit_team_obs reads.
 *   agent == 0 .. 3   dist_dev int8 [n_envs][4], 4-byte aligned: that agent's four readings on the CURRENT state; the form for use after
 *                     pmx_step_agent(agent), pmx_observe or pmx_reset.
 * n = (int)(((uint64_t)h * 13) >> 32) - 6 with h = h(PMX_SALT_SONAR), the generator documented at PMX_ACTION_APPROXQ_OFFENSE with
 * `agent` = 4 a + i and `ticks` = the env's ticks word at the time of the call.  For an enemy target this is the very draw
 * pmx_belief_update makes: after the same pmx_step r[a_j][e_k] equals its sonar_dev[row][j][k] on every row that is not reset.
 * Distribution-equivalent to noisyDistance; a reading may be negative.  The call changes nothing in the handle; an open profile records
 * the launch with the rule launches.  PMX_ERR_INVALID for a NULL handle or pointer, an agent outside -1 .. 3 or a misaligned dist_dev. */
#define PMX_OBS_SIGHT_OFF (-1)
int pmx_set_obs_sight(pmx_env *env, int32_t sight_range);
int pmx_agent_distances(pmx_env *env, int agent, int8_t *dist_dev, void *stream);

/* The layout each env is currently on (host output [n_envs]; all zeros for a single-layout handle).  Synchronises the stream. */
int pmx_get_layout_index(pmx_env *env, int32_t *index_out, void *stream);

/* Host copies of `count` games starting at `first`.  These two calls synchronise the stream. */
int pmx_get_state(pmx_env *env, int32_t first, int32_t count, pmx_state *states, void *stream);
int pmx_set_state(pmx_env *env, int32_t first, int32_t count, const pmx_state *states, void *stream);

/* distanceCalculator.computeDistances (distanceCalculator.py:111-150) for the env's layout.  cells_dev
 * [n_cells][2] int8 receives the open cells in Grid.asList(False) order (game.py:225-230), dist_dev
 * [n_cells][n_cells] uint8 the shortest 4-neighbour path lengths (255 = unreachable).  *n_cells is a host
 * output available on return (the count is computed on the host); dist_dev may be NULL to query it. */
int pmx_maze_distances(pmx_env *env, int8_t *cells_dev, uint8_t *dist_dev, int32_t *n_cells, void *stream);
/* the same for layout `layout` of a multi-layout handle */
int pmx_maze_distances_layout(pmx_env *env, int32_t layout, int8_t *cells_dev, uint8_t *dist_dev, int32_t *n_cells, void *stream);

/* Measurement hooks (no reference counterpart): between begin and end, every tick attaches a start and a stop HIP event
 * to its rule-kernel and to its expansion-kernel dispatch on the caller's stream (hipExtLaunchKernelGGL); end
 * synchronises them and returns the summed kernel durations (milliseconds) and launch counts.  bench.py's roofline
 * figures come from here.  A pmx_emit_team_obs or pmx_emit_team_obs_mixed launch (or its _fog form) is recorded with the expansion launches (a
 * training loop calls it in place of the four-agent expansion).
 * While a profile is open pmx_step runs the FULL expansion: outside one it stores the wall plane (plane 0, a per-layout
 * constant) from extra blocks of the rule launch and starts the expansion kernel behind it (float32 planes up to 900 MB, no
 * redraw_layouts).  The expansion duration reported here, which bench.py divides all plane bytes by, is therefore that of the
 * full-plane kernel -- the one pmx_reset, pmx_observe and pmx_step_agent run -- while a timed loop of plain pmx_step calls
 * measures the split tick.  The results of a tick are the same either way. */
int pmx_profile_begin(pmx_env *env, int32_t max_launches);
/* Launch tuning of the observation-expansion kernel for measurements (no reference counterpart).  The keys are "fused_min_envs" and "expand_alt"
 * (1 = walk the planes in alternating directions from tick to tick, the default; 0 = always the same direction, so that every
 * byte reaches HBM even when the caller re-steps one buffer that partly fits the Infinity Cache); any other key is an error.
 * value -1 restores the built-in choice.  "fused_min_envs": see pmx_last_step_fused. */
int pmx_set_tuning(pmx_env *env, const char *key, int32_t value);
/* 1 when the last pmx_step ran the whole tick in one launch (pmx_tick_fused_kernel), 0 when it ran the rule and the expansion
 * launch.  pmx_step takes the one launch for float32 planes up to 900 MB of all four agents, one shared layout, no bots, no
 * redraw_layouts, a board of at most 20 rows, n_envs a multiple of 64 and at least "fused_min_envs", and no open profile.
 * "fused_min_envs" is a launch threshold set with pmx_set_tuning; its default (-1) is 64 x the device's compute units, one
 * workgroup of 64 envs per unit.  The results of a tick are the same either way. */
int pmx_last_step_fused(const pmx_env *env);
int pmx_profile_end(pmx_env *env, double *rule_ms, int32_t *rule_launches, double *expand_ms, int32_t *expand_launches);

/* pacman_mappo_resnet.compute_gae (pacman_mappo_resnet.py:277-290) for n independent series laid out
 * [T][n] (time-major): rewards/values/dones float32, last_value [n] float32; adv/ret [T][n] float32. */
int pmx_gae(const float *rewards_dev, const float *values_dev, const float *dones_dev, const float *last_value_dev,
            int32_t T, int32_t n, double gamma, double lam, float *adv_dev, float *ret_dev, void *stream);

/* Column sums of a [rows][C] bfloat16 matrix as PMX_COLSUM_BLOCKS partial rows of float32 (the caller adds them): the
 * bias gradients `grad_output.sum((0, 1))` of the token linears in the critic's encoder layers (nn.TransformerEncoderLayer
 * backward, pacman_mappo_resnet.py:138-141).  C a multiple of 8, at most 256. */
#define PMX_COLSUM_BLOCKS 512
int pmx_colsum_bf16(const void *x_dev, int64_t rows, int32_t C, float *partial_dev, void *stream);

/* Training-side observation post-processing on [n][8][H][W] blocks of obs_dtype elements, for callers that take the four
 * observations of pmx_step and post-process them the way the reference script does (pacman_mappo_resnet.py:215-229
 * canonicalize_obs for a red learner, :267-274 merge_obs_for_critic): pmx.trainer.canonicalize_obs / merge_obs on device
 * tensors.  (The training loop itself gets both from pmx_emit_team_obs, already written into its rollout buffers.) */
int pmx_canonicalize_obs(const void *in_dev, void *out_dev, int32_t n, int32_t H, int32_t W, int32_t obs_dtype,
                         void *stream);
int pmx_merge_obs(const void *a_dev, const void *b_dev, void *out_dev, int32_t n, int32_t H, int32_t W,
                  int32_t obs_dtype, void *stream);

/* Fused residual add + LayerNorm over a feature dimension of 32 (the critic's post-LN encoder layers,
 * pacman_mappo_resnet.py:138-141: norm(x + sublayer(x))): y = LayerNorm(x + a) * w + b on [rows][32] tensors of float32
 * (dtype 0) or bfloat16 (dtype 1); mean / rstd [rows] float32 are saved for the backward pass.  The backward pass
 * returns dz = d loss / d (x + a) (the gradient of both inputs) and per-wavefront partial sums of the weight / bias
 * gradients: partial_dev [PMX_LN32_PARTIAL_ROWS][64] float32 (dw in columns 0..31, db in 32..63), fully overwritten;
 * the caller sums the rows. */
#define PMX_LN32_PARTIAL_ROWS 2048
int pmx_ln32_forward(const void *x_dev, const void *a_dev, const float *w_dev, const float *b_dev, void *y_dev, float *mean_dev,
                     float *rstd_dev, int64_t rows, float eps, int32_t dtype, void *stream);
int pmx_ln32_backward(const void *x_dev, const void *a_dev, const void *dy_dev, const float *w_dev, const float *mean_dev,
                      const float *rstd_dev, void *dz_dev, float *partial_dev, int64_t rows, int32_t dtype, void *stream);

/* Fused GroupNorm (8 channels per group) + optional residual add + exact GELU on [B][groups*8][H*W] tensors (NCHW),
 * the elementwise tail of the actor's residual blocks (pacman_mappo_resnet.py:58-67): y = GELU(GN(h) * w + b (+ res)).
 * dtype 0 float32, 1 bfloat16; res_dev / dres_dev may both be NULL.  Backward writes dh (and dres) and
 * partial_dev [B*groups][8][2] float32 = per (sample, group, channel) sums of dz*xhat and dz, which the caller adds up
 * over the batch to get the weight and bias gradients. */
int pmx_gn8_gelu_forward(const void *h_dev, const void *res_dev, const float *w_dev, const float *b_dev, void *y_dev, float *mean_dev,
                         float *rstd_dev, int64_t B, int32_t groups, int32_t HW, float eps, int32_t dtype, void *stream);
int pmx_gn8_gelu_backward(const void *h_dev, const void *res_dev, const void *dy_dev, const float *w_dev, const float *b_dev,
                          const float *mean_dev, const float *rstd_dev, void *dh_dev, void *dres_dev, float *partial_dev, int64_t B,
                          int32_t groups, int32_t HW, int32_t dtype, void *stream);

/* The same for channels-last bfloat16 tensors ([B][H*W][groups*8] in memory: what MIOpen's NHWC convolutions read and write). */
int pmx_gn8cl_gelu_forward(const void *h_dev, const void *res_dev, const float *w_dev, const float *b_dev, void *y_dev, float *mean_dev,
                           float *rstd_dev, int64_t B, int32_t groups, int32_t HW, float eps, void *stream);
int pmx_gn8cl_gelu_backward(const void *h_dev, const void *res_dev, const void *dy_dev, const float *w_dev, const float *b_dev,
                            const float *mean_dev, const float *rstd_dev, void *dh_dev, void *dres_dev, float *partial_dev, int64_t B,
                            int32_t groups, int32_t HW, void *stream);

/* Self-attention forward of the critic's encoder layers (nn.MultiheadAttention, embed 32, 4 heads of 8,
 * pacman_mappo_resnet.py:138-141) on the matrix cores: qkv_dev [S][B][96] bfloat16 = packed in-projection output,
 * out_dev [S][B][32] bfloat16 = concatenated heads before the out-projection, lse_dev [B][4][S] float32 (may be NULL).
 * S <= 1024. */
int pmx_attn8_forward(const void *qkv_dev, void *out_dev, float *lse_dev, int32_t S, int32_t B, void *stream);
/* Its backward pass: dqkv_dev [S][B][96] bfloat16 from the saved qkv, out, lse and the incoming dout [S][B][32].  S <= 640. */
int pmx_attn8_backward(const void *qkv_dev, const void *out_dev, const void *dout_dev, const float *lse_dev, void *dqkv_dev,
                       int32_t S, int32_t B, void *stream);
/* The same two kernels on batch-major tensors when batch_major != 0: qkv [B][S][96], out / dout [B][S][32], dqkv [B][S][96]
 * (lse stays [B][4][S]).  That is the memory order of a channels-last convolution output [B][H][W][32] read as tokens, so the
 * critic (pacman_mappo_resnet.py:160-170: projector -> flatten(2).permute(2, 0, 1) -> encoder) needs no transposing copy
 * between its convolution and its encoder layers, and a sample's rows are contiguous for the kernels. */
int pmx_attn8_forward_layout(const void *qkv_dev, void *out_dev, float *lse_dev, int32_t S, int32_t B, int32_t batch_major, void *stream);
int pmx_attn8_backward_layout(const void *qkv_dev, const void *out_dev, const void *dout_dev, const float *lse_dev, void *dqkv_dev,
                              int32_t S, int32_t B, int32_t batch_major, void *stream);

/* The PPO minibatch objective (pacman_mappo_resnet.py:571-585) and its gradient with respect to the network outputs in one
 * launch: logits_dev [B][5] float32 (logits_bf16 = 0) or bfloat16 (1); values_dev [BV] float32 with BV == B, or BV == B / 2 for
 * paired minibatches (rows 2k, 2k + 1 are the two learners of one env-tick and share value k); act_dev [B] int64; old_logp,
 * adv, ret [B] float32.  clip_eps / ent_coef come from the device pointers when those are not NULL (graph replay: the schedule
 * changes them between replays), else from the host values.  Writes stats_dev[0..4] = policy loss, value loss, mean entropy,
 * clip fraction, total loss (pg + vf_coef * vl - ent_coef * entropy), dlogits_dev [B][5] (the logits' type) and dvalues_dev
 * [BV] float32 = d total / d outputs.  The advantages are normalised per minibatch with the unbiased standard deviation (:577). */
int pmx_ppo_loss(const void *logits_dev, int32_t logits_bf16, const float *values_dev, const int64_t *act_dev,
                 const float *old_logp_dev, const float *adv_dev, const float *ret_dev, int32_t B, int32_t BV,
                 const float *clip_eps_dev, const float *ent_coef_dev, float clip_eps, float ent_coef, float vf_coef,
                 float *stats_dev, void *dlogits_dev, float *dvalues_dev, void *stream);

/* Legal-action masks for the policy (opt-in; the default path samples from all five logits, as the reference does).  One int32
 * word per row: bit a set = action a legal (0 N, 1 E, 2 S, 3 W, 4 Stop; the bits of pmx_step_out.legal_dev, widened from uint8 to
 * int32 because pmx_gather_rows moves rows in multiples of 4 bytes, and in the learner's canonical frame).  Only the low five bits
 * are read, a NULL mask pointer means everything is legal, and bit 4 (Stop) is always treated as set.
 * Stale masks: the env's masks describe the state at the START of a tick.  An agent eaten by an earlier mover of the same tick acts
 * from its start cell under a mask computed for the cell it stood on; the env's illegal-becomes-Stop rule then applies to what it
 * chose.  The objective stays consistent because it is evaluated under the stored mask the action was drawn under.
 *
 * pmx_policy_sample: one action per row of logits_dev [B][5] (float32, or bfloat16 when logits_bf16 != 0), one thread per row,
 * float32 arithmetic: z_k = the logit, or -inf where action k is masked out; zmax = max_k z_k; p_k = expf(z_k - zmax);
 * total = p_0 + ... + p_4 added in that order; logp = (z_a - zmax) - logf(total).  The draw is counter based, like the bots':
 *     h = lowbias32(seed ^ row * 0x9E3779B1 ^ counter * 0x85EBCA77 ^ 0x6A09E667),  t = (float)(h >> 8) * 0x1p-24f * total;
 * the action is the first legal k whose running sum p_0 + ... + p_k exceeds t, the last legal k if none does.  greedy != 0: the
 * legal action with the largest z, the lowest index on ties, no draw.  The same (seed, counter) on the same inputs gives the same
 * bits.  action_dev [B] int64; logp_dev [B] float32, may be NULL.  A null logits or action pointer or B < 0 is PMX_ERR_INVALID;
 * B == 0 is PMX_OK, with nothing launched or written. */
int pmx_policy_sample(const void *logits_dev, int32_t logits_bf16, const int32_t *legal_dev, int64_t B, uint32_t seed,
                      uint32_t counter, int32_t greedy, int64_t *action_dev, float *logp_dev, void *stream);
/* pmx_ppo_loss under masks: the effective mask of row i is legal_dev[i] | 1 << act_dev[i] | 0x10 (a stored action is never treated
 * as illegal).  Illegal logits enter as -inf: out of the log-sum-exp, probability 0, nothing added to the entropy, dlogits exactly
 * 0.  With every bit set (or legal_dev NULL) the outputs are pmx_ppo_loss's bit for bit. */
int pmx_ppo_loss_masked(const void *logits_dev, int32_t logits_bf16, const float *values_dev, const int64_t *act_dev,
                        const int32_t *legal_dev, const float *old_logp_dev, const float *adv_dev, const float *ret_dev, int32_t B,
                        int32_t BV, const float *clip_eps_dev, const float *ent_coef_dev, float clip_eps, float ent_coef,
                        float vf_coef, float *stats_dev, void *dlogits_dev, float *dvalues_dev, void *stream);

/* Minibatch assembly in one launch: for t < n (n <= 8), dst[t] row r = src[t] row (idx[t][r / m] * m + r % m), m =
 * rows_per_index[t], rows of row_bytes[t] bytes (a multiple of 4; multiples of 16 need 16-byte aligned bases), n_rows[t] output
 * rows.  The arrays of pointers and sizes are HOST arrays; the pointers in them are device pointers.  (What
 * pacman_mappo_resnet.py:560-569 does with `batch_indices` on its CPU tensors.) */
int pmx_gather_rows(int32_t n, const void *const *src_dev, void *const *dst_dev, const int64_t *const *idx_dev,
                    const int32_t *row_bytes, const int32_t *rows_per_index, const int64_t *n_rows, void *stream);
/* The same launch also writes n_values <= 8 float32 host values to consecutive device words (pmx_set_floats folded in: the scalars a
 * replayed graph reads travel with the minibatch). */
int pmx_gather_rows_set_floats(int32_t n, const void *const *src_dev, void *const *dst_dev, const int64_t *const *idx_dev,
                               const int32_t *row_bytes, const int32_t *rows_per_index, const int64_t *n_rows, float *floats_dst_dev,
                               const float *values, int32_t n_values, void *stream);
/* n <= 8 float32 host values to consecutive device words, passed as kernel arguments (the scalars a replayed hipGraph reads). */
int pmx_set_floats(float *dst_dev, const float *values, int32_t n, void *stream);

/* clip_grad_norm_(max_norm) -> Adam (no weight decay, no amsgrad) -> EMA on flat float32 buffers of n elements, two launches
 * (pacman_mappo_resnet.py:587-595).  scratch_dev: PMX_OPT_PARTIALS doubles.  lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t) are read
 * from scalars_dev[0..1] when it is not NULL (graph replay), else taken from the host arguments.  grad_dev is left clipped;
 * norm_out_dev (may be NULL) receives the gradient's 2-norm before clipping.  The clip factor is torch.clamp(max_norm / (norm +
 * 1e-6), max=1), NaN included: one NaN gradient element makes every gradient, moment, weight and EMA element NaN, as
 * clip_grad_norm_ does; an infinite norm gives the factor 0 and poisons the infinite elements alone. */
#define PMX_OPT_PARTIALS 1024
int pmx_clip_adam_ema(float *grad_dev, float *param_dev, float *exp_avg_dev, float *exp_avg_sq_dev, float *ema_dev, int64_t n,
                      double *scratch_dev, const float *scalars_dev, float lr_over_bc1, float rsqrt_bc2, float beta1, float beta2,
                      float eps, float max_norm, float ema_decay, float *norm_out_dev, void *stream);
/* The same two launches with the step's loose ends folded into the second one (each pointer may be NULL): param_bf16_dev receives
 * the updated parameters rounded to bfloat16 (n elements: the copy library GEMMs read under autocast); report_sums6_dev[0..4] +=
 * reports5_dev[0..4] (the objective's five scalars, pmx_ppo_loss) and report_sums6_dev[5] += the gradient norm -- the running sums
 * a caller averages over an update.  Three small launches less at the end of a replayed 512-sample step. */
int pmx_clip_adam_ema_tail(float *grad_dev, float *param_dev, float *exp_avg_dev, float *exp_avg_sq_dev, float *ema_dev, int64_t n,
                           double *scratch_dev, const float *scalars_dev, float lr_over_bc1, float rsqrt_bc2, float beta1, float beta2,
                           float eps, float max_norm, float ema_decay, float *norm_out_dev, void *param_bf16_dev,
                           const float *reports5_dev, float *report_sums6_dev, void *stream);

/* n contiguous device tensors (float32, or bfloat16 where src_is_bf16[t]) copied / widened into dst_dev at element offsets
 * dst_offset[t], count[t] elements each, one launch per 64 tensors: the parameter gradients of a step into the flat float32
 * gradient bucket.  The four arrays are HOST arrays. */
int pmx_flatten_to_f32(int32_t n, const void *const *src_dev, const uint8_t *src_is_bf16, const int64_t *dst_offset,
                       const int32_t *count, float *dst_dev, void *stream);
/* The same with the second stage of the gradient reductions folded in: where partial_rows[t] > 0, src_dev[t] points into row 0 of a
 * float32 partial-row buffer (pmx_defer_row_sums) whose rows 1 .. partial_rows[t] lie row_stride[t] floats apart, and the
 * destination receives their sum.  partial_rows / row_stride: HOST arrays, or both NULL. */
int pmx_flatten_sum_to_f32(int32_t n, const void *const *src_dev, const uint8_t *src_is_bf16, const int32_t *partial_rows,
                           const int32_t *row_stride, const int64_t *dst_offset, const int32_t *count, float *dst_dev, void *stream);

/* ---- The actor's convolutional tower as one forward and one backward kernel ------------------------------------------
 * MAPPOAgent.actor_backbone (pacman_mappo_resnet.py:104-113 with ResidualBlock :49-67):
 *   conv3x3(8->16) GELU conv3x3(16->32) GELU 3 x [conv3x3 GroupNorm(4) GELU conv3x3 GroupNorm(4) (+x) GELU], bf16 matrix-core
 *   products with fp32 accumulation, GroupNorm and GELU in fp32 on the bf16-rounded convolution output (what bf16 autocast
 *   computes).  Domain: every board with W in 8..32, H in 3..32 and H*W <= 640 cells -- the boards on which the attention
 *   backward kernel runs too, so such a board trains without a library convolution.  The padded area H*(W+2) <= 704 then needs
 *   2 .. 44 position tiles of 16; a board runs on the smallest tile-count bucket (10, 11, 16, 28, 36, 44) that holds its own
 *   count, and every buffer size below is the bucket's.  pmx_actor_supported() returns 1 on the domain and 0 elsewhere (above 640
 *   cells, sides out of range); the other entry points then return PMX_ERR_UNSUPPORTED and callers keep the library convolutions.
 * Parameters arrive as float32 device pointers in nn.Module order: conv_w[l] is [cout][cin][3][3], l = 0,1 the stem, then
 * conv1 / conv2 of the three blocks; gn_w / gn_b [6][32] are gn1, gn2 of the three blocks. */
typedef struct {
    const float *conv_w[8];
    const float *conv_b[8];
    const float *gn_w[6];
    const float *gn_b[6];
} pmx_actor_params;
#define PMX_ACTOR_PACK_BYTES 297984    /* bf16 operand fragments of the 8 layers (forward + input-gradient order) + fp32 biases / GroupNorm affine */
#define PMX_ACTOR_GRAD_FLOATS 74496    /* backward's fp32 gradient buffer: weight-gradient tiles + bias / GroupNorm gradients */
int pmx_actor_supported(int32_t H, int32_t W);
/* bytes of the activation save area (training forward -> backward) and of backward's scratch for B samples, and of the
 * scratch an inference-only forward needs (independent of B); any of the three pointers may be NULL.  The single source of
 * these sizes: they follow the board's tile-count bucket, not its own tile count, and grow monotonically with B. */
int pmx_actor_sizes(int32_t H, int32_t W, int64_t B, int64_t *save_bytes, int64_t *scratch_bytes, int64_t *infer_scratch_bytes);
/* parameters -> pack_dev [PMX_ACTOR_PACK_BYTES]; once per optimizer step (the weights changed) or once per rollout */
int pmx_actor_pack(const pmx_actor_params *params, void *pack_dev, void *stream);
/* obs_dev [B][8][H][W] of PMX_OBS_* elements -> feat_dev [B][H*W][32] bfloat16 (channels-last; the reference's nn.Flatten order
 * is the transpose of the last two dimensions).  save_dev NULL = inference (scratch_dev then holds the blocks' skip inputs
 * between layers and is required); otherwise save_dev receives what backward needs and scratch_dev may be NULL. */
int pmx_actor_forward(const void *obs_dev, int32_t obs_dtype, const void *pack_dev, void *feat_dev, void *save_dev,
                      void *scratch_dev, int64_t B, int32_t H, int32_t W, void *stream);
/* dfeat_dev [B][H*W][32] bfloat16 -> grad_dev [PMX_ACTOR_GRAD_FLOATS] (zeroed and accumulated here, sum over the batch) */
int pmx_actor_backward(const void *obs_dev, int32_t obs_dtype, const void *pack_dev, const void *save_dev, const void *dfeat_dev,
                       void *scratch_dev, float *grad_dev, int64_t B, int32_t H, int32_t W, void *stream);
/* grad_dev -> float32 gradients in the parameters' own shapes (the pointers of `out` are written, not read) */
int pmx_actor_unpack_grads(const float *grad_dev, const pmx_actor_params *out, void *stream);

/* ---- The feed-forward half of the critic's encoder layer as one forward and one backward kernel ----------------------
 * nn.TransformerEncoderLayer(d_model 32, dim_feedforward 128, ReLU, dropout 0, norm_first False), pacman_mappo_resnet.py:138-141:
 *   y = LayerNorm(x + linear2(relu(linear1(x))))   on [tokens][32] bfloat16 rows, fp32 accumulation and LayerNorm.
 * Parameters are float32 device pointers with nn.Module shapes (linear1.weight [128][32], linear2.weight [32][128], norm2). */
/* The backward kernels of this family sum their parameter gradients in two stages (a partial row per workgroup, then a row sum;
 * float atomics from every workgroup onto the same few thousand addresses are an order of magnitude slower): grad_dev must
 * hold (1 + PMX_GRAD_PARTIAL_ROWS) rows of *_GRAD_FLOATS floats; the result is row 0. */
#define PMX_GRAD_PARTIAL_ROWS 512
#define PMX_FFN_PACK_BYTES 33664
#define PMX_FFN_GRAD_FLOATS 8416      /* dW2 [32][128], dW1 [128][32], db1 [128], db2 [32], dgamma [32], dbeta [32] */
int pmx_ffn_pack(const float *w1, const float *b1, const float *w2, const float *b2, const float *gamma, const float *beta,
                 void *pack_dev, void *stream);
int pmx_ffn_forward(const void *x_dev, const void *pack_dev, void *y_dev, int64_t tokens, float eps, void *stream);
/* recomputes the forward from x (nothing is saved): dx_dev [tokens][32] bfloat16, grad_dev [1 + PMX_GRAD_PARTIAL_ROWS][PMX_FFN_GRAD_FLOATS] (row 0 = result) */
int pmx_ffn_backward(const void *x_dev, const void *dy_dev, const void *pack_dev, void *dx_dev, float *grad_dev, int64_t tokens,
                     float eps, void *stream);

/* The other token-parallel pieces of the encoder layer (nn.MultiheadAttention's packed in-projection and its out-projection
 * followed by the residual add and norm1), same kernel scheme, [tokens][32] bfloat16 inputs:
 *   tok96:    qkv [tokens][96] = in_proj_weight [96][32] a + in_proj_bias
 *   tok32ln:  y [tokens][32]  = LayerNorm(x + out_proj.weight [32][32] a + out_proj.bias)
 * Backward returns da (and dx = the gradient of the residual input) and the parameter gradients in row 0 of grad_dev
 * [1 + PMX_GRAD_PARTIAL_ROWS][*_GRAD_FLOATS]:
 *   tok96:   dW [96][32], db [96]                  (+ 64 unused floats)
 *   tok32ln: dW [32][32], db [32], dgamma [32], dbeta [32] */
#define PMX_TOK96_PACK_BYTES 12928
#define PMX_TOK96_GRAD_FLOATS 3232
#define PMX_TOK32_PACK_BYTES 4480
#define PMX_TOK32_GRAD_FLOATS 1120
int pmx_tok96_pack(const float *w, const float *b, void *pack_dev, void *stream);
int pmx_tok96_forward(const void *a_dev, const void *pack_dev, void *y_dev, int64_t tokens, void *stream);
int pmx_tok96_backward(const void *a_dev, const void *dy_dev, const void *pack_dev, void *da_dev, float *grad_dev, int64_t tokens, void *stream);
/* pmx_tok96_backward with da = in_proj_weight^T dy + res: res_dev [tokens][32] bfloat16 (or NULL) is the gradient that reaches the same
 * tokens through the residual connection of the encoder layer (nn.TransformerEncoderLayer: norm1(x + self_attn(x)), pacman_mappo_resnet.py:
 * 138-141) -- autograd would add the two with a kernel of its own.  res_dev must not be da_dev. */
int pmx_tok96_backward_res(const void *a_dev, const void *dy_dev, const void *pack_dev, const void *res_dev, void *da_dev, float *grad_dev,
                           int64_t tokens, void *stream);
int pmx_tok32ln_pack(const float *w, const float *b, const float *gamma, const float *beta, void *pack_dev, void *stream);
int pmx_tok32ln_forward(const void *x_dev, const void *a_dev, const void *pack_dev, void *y_dev, int64_t tokens, float eps, void *stream);
int pmx_tok32ln_backward(const void *x_dev, const void *a_dev, const void *dy_dev, const void *pack_dev, void *dx_dev, void *da_dev,
                         float *grad_dev, int64_t tokens, float eps, void *stream);

/* ---- The small ends of the two heads, one kernel each way (csrc/pmx_heads.hip) ----------------------------------------
 * Actor tail (pacman_mappo_resnet.py:117-122, actor_head[1:]): logits = W2 gelu(LayerNorm_512(h)) + b2 on the 512-wide output h
 * [B][512] (bfloat16 if h_bf16, else float32) of the first head layer; logits_dev [B][5] float32; stats_dev [B][2] float32 (mean,
 * rstd; may be NULL for inference).  Backward: dh_dev [B][512] in h's type, and the parameter gradients in row 0 of grad_dev
 * [1 + PMX_HEADS_PARTIAL_ROWS][PMX_ACTOR_TAIL_GRAD_FLOATS]: dW2 [5][512], db2 [5] (+ 3 unused), dLN.weight [512], dLN.bias [512].
 * Critic tail (:143-147 critic_head on the mean over tokens, :169): value = w2 gelu(W1 mean_s tokens[b][s] + b1) + b2 with tokens
 * [B][S][32] bfloat16 (the batch-major encoder output); pooled_dev [B][32] float32 is saved for backward.  Backward: dtokens_dev
 * [B][S][32] bfloat16, scratch_dev 2 * B * 512 bfloat16, row 0 of grad_dev [1 + PMX_HEADS_PARTIAL_ROWS][PMX_CRITIC_TAIL_GRAD_FLOATS]: dW1
 * [512][32], db1 [512], dw2 [512], db2 [1] (+ 7 unused).  Parameters are float32 device pointers with nn.Module shapes; the kernels round the two linears' weights
 * and inputs to bfloat16 as autocast does and keep LayerNorm / GELU in float32. */
#define PMX_HEADS_PARTIAL_ROWS 128
#define PMX_ACTOR_TAIL_GRAD_FLOATS 3592
#define PMX_CRITIC_TAIL_GRAD_FLOATS 17416
int pmx_actor_tail_forward(const void *h_dev, int32_t h_bf16, const float *ln_w, const float *ln_b, const float *w2, const float *b2,
                           float *logits_dev, float *stats_dev, int64_t B, float eps, void *stream);
int pmx_actor_tail_backward(const void *h_dev, int32_t h_bf16, const float *stats_dev, const float *dlogits_dev, const float *ln_w,
                            const float *ln_b, const float *w2, void *dh_dev, float *grad_dev, int64_t B, void *stream);
int pmx_critic_tail_forward(const void *tokens_dev, const float *w1, const float *b1, const float *w2, const float *b2,
                            float *value_dev, float *pooled_dev, int64_t B, int32_t S, void *stream);
int pmx_critic_tail_backward(const float *pooled_dev, const float *dvalue_dev, const float *w1, const float *b1, const float *w2,
                             void *dtokens_dev, void *scratch_dev, float *grad_dev, int64_t B, int32_t S, void *stream);

/* ---- The first layer of the actor head on the matrix cores (csrc/pmx_actor_head.hip) ---------------------------------------
 * MAPPOAgent.actor_head[0], Linear(32 H W -> 512) (pacman_mappo_resnet.py:117-119), between pmx_actor_forward and pmx_actor_tail_forward,
 * on the boards pmx_actor_supported() accepts (PMX_ERR_UNSUPPORTED elsewhere; a null pointer or B < 0: PMX_ERR_INVALID; B == 0: PMX_OK,
 * nothing is launched or written):
 *   w         [512][32 H W] float32, the parameter as nn.Linear stores it (column ch * HW + cell); bias, db_dev [512] float32
 *   feat_dev, dfeat_dev [B][H W][32] bfloat16 (what pmx_actor_forward writes and pmx_actor_backward reads; contraction index cell * 32 + ch)
 *   h_dev, dh_dev       [B][512] bfloat16 (what pmx_actor_tail_forward / _backward take and return with h_bf16 = 1)
 *   dw_dev    [512][32 H W] float32 in the parameter's own order, written in full
 * pmx_actor_head_sizes (host only) gives the bytes of the packed operand images pmx_actor_head_pack writes (the weight rounded to
 * bfloat16 once, cell-major, and its transpose) and of the scratch either direction needs for B samples (both 16-byte aligned).
 * Products are v_mfma_f32_16x16x32_bf16 with float32 accumulation; the bias is added in float32 before the single rounding of h; dw and
 * db stay float32.  Partial sums (split K forward, split batch in the weight gradient) go to slabs in the scratch and are added in a
 * fixed order: no atomics, the same call on the same inputs returns the same bits.  B above PMX_ACTOR_HEAD_MAX_BATCH (row indices and
 * grid sizes stay inside 32 bits): PMX_ERR_UNSUPPORTED. */
#define PMX_ACTOR_HEAD_MAX_BATCH 4194304
int pmx_actor_head_sizes(int32_t H, int32_t W, int64_t B, int64_t *pack_bytes, int64_t *scratch_bytes);   /* pacman_mappo_resnet.py:117-119 */
int pmx_actor_head_pack(const float *w, void *pack_dev, int32_t H, int32_t W, void *stream);              /* pacman_mappo_resnet.py:117-119 */
int pmx_actor_head_forward(const void *feat_dev, const void *pack_dev, const float *bias, void *h_dev, void *scratch_dev, int64_t B,
                           int32_t H, int32_t W, void *stream);                                           /* pacman_mappo_resnet.py:117-119 */
int pmx_actor_head_backward(const void *feat_dev, const void *dh_dev, const void *pack_dev, void *dfeat_dev, float *dw_dev, float *db_dev,
                            void *scratch_dev, int64_t B, int32_t H, int32_t W, void *stream);            /* pacman_mappo_resnet.py:117-119 */

/* All parameter packs of up to four encoder layers in one launch (what pmx_tok96_pack, pmx_tok32ln_pack and pmx_ffn_pack produce, into
 * the three pack buffers of each layer). */
typedef struct {
    const float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b, *norm1_w, *norm1_b;     /* [96][32], [96], [32][32], [32], [32], [32] */
    const float *lin1_w, *lin1_b, *lin2_w, *lin2_b, *norm2_w, *norm2_b;                   /* [128][32], [128], [32][128], [32], [32], [32] */
    void *pack_in, *pack_out, *pack_ffn;    /* PMX_TOK96_PACK_BYTES, PMX_TOK32_PACK_BYTES, PMX_FFN_PACK_BYTES */
} pmx_encoder_layer_params;
int pmx_encoder_pack(int32_t n_layers, const pmx_encoder_layer_params *layers, void *stream);

/* ---- The critic's projector: conv3x3(8 -> 32) + bias + 2-D positional encoding -> batch-major tokens ---------------------
 * MAPPOAgent.critic_projector and pos_encoder (pacman_mappo_resnet.py:126-127, :69-95, :164) on boards pmx_actor_supported() accepts
 * (W in 8..32, H in 3..32, H*W <= 640; PMX_ERR_UNSUPPORTED elsewhere):
 * obs_dev [B][8][H][W] of PMX_OBS_* elements -> tokens_dev [B][H*W][32] bfloat16 (what flatten(2).permute(2, 0, 1) yields, batch-major),
 * bf16 products with fp32 accumulation, the convolution (+ bias) rounded to bfloat16 before the table (posenc_dev [H*W][32] float32) is
 * added in bfloat16, as autocast computes it.  Backward returns the weight and bias gradients only (the observations need none):
 * dw_dev [32][8][3][3], db_dev [32] float32; partial_dev is scratch of PMX_PROJ_PARTIAL_ROWS x PMX_PROJ_GRAD_ROW_FLOATS floats. */
#define PMX_PROJ_PACK_BYTES 6272
#define PMX_PROJ_PARTIAL_ROWS 256
#define PMX_PROJ_GRAD_ROW_FLOATS 2592
int pmx_proj_pack(const float *w, const float *b, void *pack_dev, void *stream);
int pmx_proj_forward(const void *obs_dev, int32_t obs_dtype, const void *pack_dev, const float *posenc_dev, void *tokens_dev, int64_t B,
                     int32_t H, int32_t W, void *stream);
int pmx_proj_backward(const void *obs_dev, int32_t obs_dtype, const void *dtokens_dev, float *partial_dev, float *dw_dev, float *db_dev,
                      int64_t B, int32_t H, int32_t W, void *stream);

/* Deferred row sums (per host thread).  The backward entry points of the pmx_ffn / pmx_tok96 / pmx_tok32ln / pmx_actor_tail / pmx_critic_tail
 * families end with a small second-stage kernel that adds their partial rows into row 0 of grad_dev.  After pmx_defer_row_sums(1) they
 * skip it; pmx_last_partial_rows() then tells how many rows the last such call left (0: row 0 is already final), and the caller adds them
 * with pmx_sum_partial_rows(grad_dev, rows, floats-per-row, stream) -- on a side stream, beside the next backward kernel. */
int pmx_defer_row_sums(int32_t on);
int pmx_last_partial_rows(void);
int pmx_sum_partial_rows(float *buf_dev, int32_t n_rows, int32_t floats, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PMX_H */
