// pmx_device.h -- structures shared by the HIP kernels and the C-ABI host code (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PMX_BLOCK 256            // expansion kernel: 4 wavefronts of 64
#define PMX_RULE_BLOCK 64        // rule kernels: one wavefront per block, so that N/64 blocks spread over all CUs
#define PMX_WALL_BLOCKS 1024     // pmx_rule_kernel: one-wave blocks appended to the grid that store the wall plane (4 per CU)
#define PMX_F32_STREAM_BYTES ((size_t)900 << 20)   // float32 planes beyond this take the streaming expansion (pmx_launch_expand)
#define PMX_SCARED_TIME 40       // capture.py:75
#define PMX_MIN_FOOD 2           // capture.py:70

// ---------------------------------------------------------------------------------------------
// Device state layout: structure-of-arrays of 32-bit words, word-major: state[word * N + env].
// One lane owns one env in the rule kernel, so every access below is a fully coalesced dword stream.
//   [0, H)        food rows, bit x of row y
//   H + i         agent i word A: x | y << 8 | dir << 16 | isPacman << 24
//   H + 4 + i     agent i word B: scaredTimer | numCarrying << 8 (12 bits) | numReturned << 20 (12 bits)
//   H + 8, H + 9  capsule list: four 16-bit slots (x | y << 8), 0xFFFF = empty
//   H + 10        score (int32)
//   H + 11        steps (int32)
//   H + 12        ticks since creation (never reset): counter of the PMX_ACTION_RANDOM_LEGAL generator
//   H + 13 ...    accumulators of an open tick, used only by pmx_step_agent:
//                 red reward (2 words, f64), blue reward (2 words), red score change, blue score change, total
// A "snapshot" is the first H + 10 words of this layout; the observation encoder reads snapshots.
// ---------------------------------------------------------------------------------------------
#define PMX_W_AGENT_A(H, i) ((H) + (i))
#define PMX_W_AGENT_B(H, i) ((H) + 4 + (i))
#define PMX_W_CAPS(H, j) ((H) + 8 + (j))
#define PMX_W_SCORE(H) ((H) + 10)
#define PMX_W_STEPS(H) ((H) + 11)
#define PMX_W_TICKS(H) ((H) + 12)
#define PMX_W_ACC(H) ((H) + 13)
#define PMX_SNAP_WORDS(H) ((H) + 10)
#define PMX_STATE_WORDS(H) ((H) + 20)

struct PmxLayoutDev {
    int32_t W, H, half;          // half = int(W / 2): the food split (capture.py:333)
    uint32_t lo_mask, hi_mask;   // columns x < half / x >= half
    uint32_t walls[32];
    uint32_t food0[32];
    uint32_t capw0[2];
    int32_t startx[4], starty[4];
    int32_t total_food;
    int32_t n_dump;              // entries of the dump-order table
    uint32_t wall_stream[32];    // plane 0 of the observation as a packed bit stream: bit (y*W + x) = wall
    int32_t n_cells;             // open cells (rows of this layout's maze-distance matrix)
    uint32_t dist_off;           // byte offset of that matrix in the handle's distance buffer
};

struct PmxTickParams {
    uint32_t *state;             // [PMX_STATE_WORDS][N]
    uint32_t *snap;              // [3][PMX_SNAP_WORDS][N] states after sub-steps 0,1,2
    const PmxLayoutDev *lay;     // [n_layouts]
    const int32_t *layout_idx;   // [N] layout of each env, or NULL when the handle has one layout
    const int8_t *dump;          // [n_dump][2] BFS visit order of dumpFoodFromDeath
    const int8_t *actions;
    int32_t N, length, legal_reward, defence_reward, auto_reset;
    double *reward;
    uint8_t *done;
    uint8_t *legal;
    int32_t *score_change;
    int32_t *score;
    const uint8_t *dist;         // maze-distance matrices of all layouts (in-kernel baselineTeam bots), or NULL
    const int16_t *cell_index;   // [n_layouts][32*32] cell -> row of the distance matrix
    uint32_t *agent_out;         // [N][4] x | y<<8 | carry<<16 right after the agent's own sub-step
    uint32_t seed;
    const uint8_t *reset_mask;   // reset kernel only: NULL = every env
    int32_t no_reset;            // reset kernel only: 1 = touch no env (legal masks of the current state only)
    // host-side copies of what every layout of a handle shares, so that the kernel has them with its arguments instead
    // of behind a dependent load from the layout record
    int32_t lay_W, lay_H, lay_half, lay_n_dump;
    uint32_t lo_mask, hi_mask;
    int32_t *layout_idx_rw;      // the same array as layout_idx when envs move to a new layout at every reset (redraw), else NULL
    int32_t n_layouts;
    // pmx_rule_kernel only: blocks with blockIdx.x >= rule_blocks store the vectors that lie wholly inside plane 0 (the walls,
    // a per-layout constant) of every (env, emitted agent) block of obs while the rule blocks run.  obs == NULL: no such blocks
    float *obs;                  // [N][n_emit][8][H][W], float32 planes only
    int32_t n_emit;
    int32_t rule_blocks;
    int32_t bot_sight;           // 0: the bots keep the full state; 1 .. PMX_SIGHT_RANGE_MAX: the sight instantiations (pmx_set_bot_sight)
};

struct PmxExpandParams {
    const uint32_t *snap[4];     // per AGENT: base of the snapshot its planes are encoded from
    const PmxLayoutDev *lay;     // [n_layouts]
    const int32_t *layout_idx;   // [N] or NULL
    void *obs;                   // [N][n_emit][8][H][W]
    int32_t N, n_emit;
    int32_t emit[4];             // agent index of each emitted slot
    int32_t single_agent;        // >= 0: obs is [N][8][H][W] for that agent only (pmx_step_agent)
    int32_t lay_H, lay_W;        // host-side copies of the common layout dimensions (launch sizing)
    int32_t reverse;             // 1: walk the blocks from the highest address down (alternate ticks, see pmx_launch_expand)
    int32_t first_vec;           // pmx_expand_kernel<0, false, true>: number of 16-byte vectors wholly inside plane 0, H*W*4/16.  0: the
                                 // kernel stores the whole block; otherwise the rule launch (PmxTickParams::obs) stored the block's
                                 // first wall_split_vec(block, first_vec) vectors and the kernel starts behind them
};

// Where a float32 (env, agent) block is split between the wall writer (streaming stores) and the expansion (ordinary stores):
// the largest s <= first_vec for which block + 16 s is a multiple of 128, or 0 if there is none.  first_vec = H*W*4/16 is the
// number of vectors wholly inside plane 0; the vectors s .. first_vec - 1 hold walls only and the expansion stores them from its
// stream table.  With the split on a 128-byte line of the ADDRESS every 1 KiB store instruction behind it covers 8 whole lines,
// and no 64-byte granule is written half by a streaming and half by an ordinary store.  The writer and the reader of a block
// both call this with the block's own address, so a buffer of any (16-byte) alignment is split consistently.
__host__ __device__ inline int wall_split_vec(const void *block, int first_vec)
{
    const int s = first_vec - (int)(((uintptr_t)block / 16 + (uintptr_t)first_vec) & 7);
    return s > 0 ? s : 0;
}

// pmx_emit_team_obs: the two observations of one team, canonicalised for a red team, + the merged critic input
struct PmxEmitParams {
    const uint32_t *snap[4];     // per agent: the snapshot its planes are encoded from (as in PmxExpandParams)
    const PmxLayoutDev *lay;
    const int32_t *layout_idx;
    void *team_obs;              // [N][2][8][H][W]
    void *merged;                // [N][8][H][W] or NULL
    int32_t N, red;              // red: agents (0, 2), x-flipped with planes 2<->3 and 6<->7 swapped; else agents (1, 3) as they are
    int32_t lay_H, lay_W;
    // pmx_emit_team_obs_mixed only (pmx_emit_team_kernel<DT, true>; zero and unread otherwise): the colour per env in place of
    // `red`, and the env range of the launch -- team_obs / merged then hold `count` rows, row j for env first + j
    const uint8_t *team_red;     // [N], non-zero = red
    int32_t first, count;
    // pmx_emit_team_obs_fog / _mixed_fog only (pmx_emit_team_kernel<DT, MIXED, true>; zero and unread otherwise): an enemy shows
    // in a learner's plane 5 only within this Manhattan distance of one of the two team agents (capture.py:285-291)
    int32_t sight;
    // pmx_emit_team_obs_belief / _mixed_belief only (pmx_emit_team_kernel<DT, MIXED, false, true>; NULL and unread otherwise): the
    // tracker's sets, [rows][2 slots][2 enemies][32] row words; learner slot j's plane 5 is the OR of its two sets
    const uint32_t *belief;
    // pmx_emit_team_obs_weighted / _mixed_weighted only (pmx_emit_team_kernel<DT, MIXED, false, false, true>; NULL and unread
    // otherwise): the weighted tracker's levels, uint8 [rows][2 slots][HW], cell y * W + x raw; learner slot j's plane 5 is
    // levels[row][j] as numbers
    const uint8_t *levels;
};

// pmx_belief_update / pmx_belief_init: the possibilistic tracker of the hidden enemies (include/pmx.h, "Belief sets")
struct PmxBeliefParams {
    const uint32_t *snap[4];     // per agent: the snapshot its planes are encoded from (as in PmxEmitParams)
    const uint32_t *state;       // the env's state words: the tick counter keys the sonar draw
    const PmxLayoutDev *lay;
    const int32_t *layout_idx;
    const uint8_t *team_red;     // [N] colour per env, or NULL: `red` for all
    const uint8_t *reset;        // [N] non-zero = back to the start cells, or NULL
    uint32_t *belief;            // [count][2][2][32]
    int8_t *sonar;               // [count][2][2] or NULL
    int32_t N, red, first, count, sight;
    int32_t lay_H, lay_W;
    uint32_t seed;
    int32_t kind;                // pmx_belief_init only: 0 = start cells, 1 = every open cell
};

// pmx_belief_weights_update / pmx_belief_weights_init (include/pmx.h, "Belief weights"): the set tracker's block, unchanged, and
// the two buffers of the weighted filter.  A block of its own, so that pmx_belief_kernel's argument is the one it was.
struct PmxBeliefWeightsParams {
    PmxBeliefParams b;
    uint16_t *weights;           // [count][2 slots][2 enemies][HW]
    uint8_t *levels;             // [count][2 slots][HW]
};

// pmx_belief_update_evidence / pmx_belief_weights_update_evidence (include/pmx.h, "Belief evidence"): the evidence kernels
// take the parents' block, unchanged, and this one as a second argument, so that the parents' argument is the one it was
struct PmxBeliefEvidenceParams {
    uint32_t *evidence;          // [count][36]: food rows 0 .. 31, P[first], P[second], valid, 0 of the last update's slot-1 snapshot
    int32_t rules;               // PMX_EVIDENCE_* bits
};

// Host-side launch tuning, changed through pmx_set_tuning: -1 = the built-in choice.
struct PmxExpandTuning {
    int32_t alt = -1;            // alternate the sweep direction from tick to tick (0: always the same direction)
    int32_t fused_min_envs = -1; // pmx_step takes the one-launch tick from this many envs on (-1: 64 x the device's CU count)
};
