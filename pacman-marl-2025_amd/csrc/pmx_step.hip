// pmx_step.hip -- the batched Capture-the-Flag tick for gfx950 (MI355X).
//
// Two kernels per tick (one, pmx_tick_fused_kernel below, where pmx_step can give a workgroup its 64 envs end to end):
//   pmx_rule_kernel    one LANE per env: the four agent sub-steps of gymPacMan.step (gymPacMan.py:143-193) with the
//                      rules of capture.py:448-728, the shaped reward of gymPacMan.py:231-259 and the termination
//                      test of gymPacMan.py:261-270.  Food rows live in LDS (one column per lane, conflict free),
//                      agents in registers.  It leaves the state after each sub-step as a coalesced SoA snapshot.
//                      In pmx_step its grid carries extra one-wave blocks that store plane 0 (the walls, the only plane
//                      that does not depend on the rules) of the observation while the rule waves wait on memory.
//   pmx_expand_kernel  one WAVEFRONT per (env, agent): turns a snapshot into the 8 observation planes of
//                      gymPacMan.get_Observation (gymPacMan.py:195-229), in pmx_step from behind the wall vectors the rule
//                      launch stored, with 16-byte-per-lane stores (ordinary while the
//                      planes can live in the Infinity Cache, walking the blocks in alternating directions from tick to
//                      tick; streaming with capped occupancy beyond).  This kernel moves >95 % of the bytes of the tick
//                      and is the HBM-roofline kernel.
// The split keeps the divergent integer rule logic at 64 envs per wave while the byte-heavy expansion gets
// N*4 wavefronts of perfectly coalesced stores regardless of N.
#include <algorithm>
#include <cstdlib>

#include <hip/hip_ext.h>

#include "pmx_device.h"
#include "pmx_belief.h"

#define PMX_MAX_H_LDS 32   // per-lane wall columns (multi-layout handles) start after room for 32 food rows

namespace {

struct Env {
    uint32_t xy[4];        // x | y << 8: one compare tests "same cell" (capture.py:682,708 collisions at tolerance 0.7)
    int dir[4], pac[4], scared[4], carry[4], ret[4];
    uint32_t capw[2];
    int score, steps;
    uint32_t ticks;        // never reset
    uint32_t self_after[4];  // x | y<<8 | carry<<16 of agent i right after its own sub-step
};

struct Acc {
    double red_r, blue_r;
    int red_sc, blue_sc, sc_total;
    int n_red, n_blue;     // pellets on the red / blue half (capture.py:332-342), kept up to date by the hot kernel only (HB > 0)
};

struct Ctx {
    const uint32_t *wl;   // LDS: wall rows, row y at wl[y * wls] (wls = 1: one shared layout; PMX_RULE_BLOCK: per-lane layouts)
    int wls;
    uint32_t *fd;         // LDS: this lane's food column, row y at fd[y * PMX_RULE_BLOCK]
    const PmxLayoutDev *L;
    const int8_t *dump;
    int W, H, half, n_dump;
    uint32_t lo_mask, hi_mask;   // halfGrid column masks of this layout (loaded once, up front)
    int legal_reward, defence_reward;
    uint32_t rng_key;     // seed ^ env * 0x9E3779B1 (the per-env part of the random-legal key)
    uint32_t start_xy[4]; // start cells, packed like Env::xy
    uint32_t *fd2;        // LDS: scratch food column for the reflex bots' what-if successors
    uint32_t *fd3;        // LDS: scratch column of dump_food (rows of cells that cannot take a pellet)
    const uint8_t *dist;  // this env's layout's maze-distance matrix (or NULL)
    const int16_t *cidx;  // its cell -> matrix row map
    int n_cells;
    uint32_t *rows0;      // LDS: row 0 of the whole block's food rows ([row][lane]; fd = rows0 + lane)
    uint32_t *stg;        // LDS: [16][PMX_RULE_BLOCK] staging words of the wide snapshot / state stores
};

__device__ __forceinline__ uint32_t pack_a(const Env &e, int i)
{
    return e.xy[i] | ((uint32_t)e.dir[i] << 16) | ((uint32_t)e.pac[i] << 24);
}
__device__ __forceinline__ uint32_t pack_b(const Env &e, int i)
{
    return (uint32_t)e.scared[i] | ((uint32_t)e.carry[i] << 8) | ((uint32_t)e.ret[i] << 20);
}
__device__ __forceinline__ void unpack_a(Env &e, int i, uint32_t w)
{
    e.xy[i] = w & 0xFFFFu; e.dir[i] = (w >> 16) & 0xFF; e.pac[i] = (w >> 24) & 1;
}
__device__ __forceinline__ void unpack_b(Env &e, int i, uint32_t w)
{
    e.scared[i] = w & 0xFF; e.carry[i] = (w >> 8) & 0xFFF; e.ret[i] = (w >> 20) & 0xFFF;
}

// capture.py:453-461 + game.py:335-350: bit a = action a legal (0 N, 1 E, 2 S, 3 W, 4 Stop)
__device__ __forceinline__ int legal_mask(const uint32_t *wl, int wls, int x, int y)
{
    uint32_t r0 = ~wl[y * wls], rn = ~wl[(y + 1) * wls], rs = ~wl[(y - 1) * wls];
    return (int)(((rn >> x) & 1u) | (((r0 >> (x + 1)) & 1u) << 1) | (((rs >> x) & 1u) << 2) |
                 (((r0 >> (x - 1)) & 1u) << 3) | (((r0 >> x) & 1u) << 4));
}

__device__ __forceinline__ int cap_find(const Env &e, uint32_t key)
{
    if ((e.capw[0] & e.capw[1]) == 0xFFFFFFFFu) return -1;      // no capsule left (the common case)
    if ((e.capw[0] & 0xFFFFu) == key) return 0;
    if ((e.capw[0] >> 16) == key) return 1;
    if ((e.capw[1] & 0xFFFFu) == key) return 2;
    if ((e.capw[1] >> 16) == key) return 3;
    return -1;
}
__device__ __forceinline__ void cap_remove(Env &e, int slot)
{
    uint32_t m = 0xFFFFu << (16 * (slot & 1));
    if (slot < 2) e.capw[0] |= m; else e.capw[1] |= m;
}

__device__ __forceinline__ void send_home(Env &e, const Ctx &c, int i)
{   // capture.py:691-693 / 699-701 / 717-719 / 725-727
    e.pac[i] = 0; e.xy[i] = c.start_xy[i]; e.dir[i] = 4; e.scared[i] = 0;
}

// capture.py:569-668 dumpFoodFromDeath.  The reference's FIFO BFS visits offsets in a board-independent order;
// c.dump holds that order (generated on the host by running the same BFS), so the walk is a linear scan.
__device__ __forceinline__ void dump_food(Env &e, const Ctx &c, uint32_t who_xy, int num, int &d_red, int &d_blue)
{
    const int who_x = who_xy & 0xFF, who_y = who_xy >> 8;
    const int side_red = 2 * who_x < c.W;
    // Three things keep this rare path short (a tick in which some env dumps food used to be 4 us slower than one without,
    // and with 16 k envs in lock-step most ticks have one): (1) the table index is wave-uniform, so the entries come through
    // the scalar cache (constant address space) -- a vector load costs an L2 round trip per candidate AND waits for the
    // snapshot stores in front of it (stores share vmcnt with loads on gfx9); (2) every test of capture.py:604-629 except
    // "inside the rows" is folded once into per-row masks of cells that cannot take a pellet (LDS scratch column fd3), so a
    // candidate costs one row read and one bit test; (3) candidates are taken four at a time (one LDS round trip per group)
    // and judged strictly in order; a pellet is placed with an LDS OR (a cell occurs once in the visit order).
    typedef const uint32_t __attribute__((address_space(4))) *const_words_t;
    const const_words_t dwords = (const_words_t)(uintptr_t)c.dump;
    // rows of cells that cannot take a pellet: walls, food, the other side (2x < W decides, :618), the border columns x = 0 and
    // x >= W (:609), capsules (:621) and agents (:625-627); row 0 and rows >= H are rejected by the index test below
    const uint32_t inner = (c.W >= 32 ? 0xFFFFFFFFu : ((1u << c.W) - 1u)) & ~1u;
    const uint32_t red_cols = (1u << ((c.W + 1) >> 1)) - 1u;                  // x with 2x < W
    const uint32_t allowed = inner & (side_red ? red_cols : ~red_cols);
    c.fd3[0] = 0xFFFFFFFFu;
    for (int y = 1; y < c.H; ++y) c.fd3[y * PMX_RULE_BLOCK] = c.wl[y * c.wls] | c.fd[y * PMX_RULE_BLOCK] | ~allowed;
#pragma unroll
    for (int i = 0; i < 4; ++i) atomicOr(&c.fd3[(e.xy[i] >> 8) * PMX_RULE_BLOCK], 1u << (e.xy[i] & 0xFF));
    if ((e.capw[0] & e.capw[1]) != 0xFFFFFFFFu) {
#pragma unroll
        for (int sl = 0; sl < 4; ++sl) {
            const uint32_t cxy = ((sl < 2 ? e.capw[0] : e.capw[1]) >> (16 * (sl & 1))) & 0xFFFFu;
            if (cxy != 0xFFFFu) atomicOr(&c.fd3[(cxy >> 8) * PMX_RULE_BLOCK], 1u << (cxy & 0xFF));
        }
    }
    for (int k = 0; k < c.n_dump && num > 0; k += 4) {
        const uint32_t w0 = dwords[k >> 1], w1 = dwords[(k >> 1) + 1];      // the table is padded with out-of-board offsets
        int X[4], Y[4];
        bool inb[4];
        uint32_t brow[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t ent = ((j < 2 ? w0 : w1) >> (16 * (j & 1))) & 0xFFFFu;
            X[j] = who_x + (int)(int8_t)(ent & 0xFF); Y[j] = who_y + (int)(int8_t)(ent >> 8);
            inb[j] = (uint32_t)Y[j] < (uint32_t)c.H && (uint32_t)X[j] < 32u;
            brow[j] = c.fd3[(inb[j] ? Y[j] : 0) * PMX_RULE_BLOCK];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (num <= 0 || !inb[j] || ((brow[j] >> X[j]) & 1u)) continue;
            atomicOr(&c.fd[Y[j] * PMX_RULE_BLOCK], 1u << X[j]);
            --num;
            if (X[j] < c.half) ++d_red; else ++d_blue;
        }
    }
}

template <int WHO>
__device__ __forceinline__ void kill_dump(Env &e, const Ctx &c, int &d_red, int &d_blue)
{
    if (e.pac[WHO] && e.carry[WHO] > 0) dump_food(e, c, e.xy[WHO], e.carry[WHO], d_red, d_blue);
    if (e.pac[WHO]) e.carry[WHO] = 0;   // (a non-Pacman here is the reference's "seriously wrong" raise: unreachable)
}

// capture.py:519-560 consume, for an eater of team RED / blue standing on (px, py)
template <bool RED>
__device__ __forceinline__ void consume(Env &e, const Ctx &c, int px, int py, int &d_red, int &d_blue)
{
    const uint32_t key = (uint32_t)px | ((uint32_t)py << 8);
    uint32_t row = c.fd[py * PMX_RULE_BLOCK];
    if ((row >> px) & 1u) {
        constexpr int T1 = RED ? 0 : 1, T2 = T1 + 2;                      // :533-537 team order
        if (e.xy[T1] == key) e.carry[T1] += 1;
        else if (e.xy[T2] == key) e.carry[T2] += 1;
        c.fd[py * PMX_RULE_BLOCK] = row & ~(1u << px);
        if (px < c.half) --d_red; else --d_blue;
    }
    int slot = cap_find(e, key);
    if (slot >= 0) {
        bool mine = RED ? (2 * px > c.W) : (2 * px <= c.W);               // halfList, capture.py:344-350
        if (mine) {
            cap_remove(e, slot);
            constexpr int O1 = RED ? 1 : 0, O2 = O1 + 2;
            e.scared[O1] = PMX_SCARED_TIME; e.scared[O2] = PMX_SCARED_TIME;
        }
    }
}

// capture.py:107-123 generateSuccessor for mover I, in place.  Returns scoreChange; d_red/d_blue receive the net
// change of the food counts on the red / blue side (what gymPacMan.get_reward compares, gymPacMan.py:234-247).
// PMX_ACTION_RANDOM_LEGAL: uniform choice among the legal actions in the reference's list order N,S,E,W,Stop
// (agents/randomTeam.py:100 random.choice(actions)); lowbias32 hash of (seed, env, tick, agent) as the generator.
__device__ __forceinline__ int random_legal(int legal, uint32_t key, uint32_t ticks, int agent)
{
    uint32_t x = key ^ (ticks * 0x85EBCA77u) ^ ((uint32_t)agent * 0xC2B2AE3Du);
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    const uint32_t n = (uint32_t)__popc(legal);
    int k = (int)(((uint64_t)x * n) >> 32);
    int pick = 4;
    const int order[5] = { 0, 2, 1, 3, 4 };
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int a = order[j];
        if ((legal >> a) & 1) { if (k == 0) pick = a; --k; }
    }
    return pick;
}

template <int I>
__device__ __forceinline__ int substep_core(Env &e, const Ctx &c, int action, bool &req_legal, int &d_red, int &d_blue)
{
    constexpr bool RED = (I % 2) == 0;
    constexpr int O1 = RED ? 1 : 0, O2 = O1 + 2;
    // ---- applyAction capture.py:468-517
    int px = e.xy[I] & 0xFF, py = e.xy[I] >> 8;
    const int legal = legal_mask(c.wl, c.wls, px, py);
    req_legal = (action >= 0) && (action <= 4) && ((legal >> (action & 7)) & 1);
    if (!req_legal) action = 4;                                           // :473-474
    px += (action == 1) - (action == 3); py += (action == 0) - (action == 2);
    e.xy[I] = (uint32_t)px | ((uint32_t)py << 8);
    if (action != 4) e.dir[I] = action;                                   // game.py:115-118
    e.pac[I] = (int)(RED != (2 * px < c.W));                              // :492
    int eater_pac = e.pac[I];
    int sc = 0;
    if (e.carry[I] > 0 && !e.pac[I]) {                                    // :495-511
        sc = RED ? e.carry[I] : -e.carry[I];
        e.ret[I] += e.carry[I];
        e.carry[I] = 0;
        eater_pac = e.pac[3];                                             // :505 leaves agentState bound to agent 3
    }
    if (eater_pac) consume<RED>(e, c, px, py, d_red, d_blue);            // :514-515
    // ---- checkDeath capture.py:670-728.  Nothing happens unless an opponent stands on the mover's cell, so the common
    // case is two compares; the sequential logic (the isPacman branch is chosen once, positions are re-read per
    // opponent because the mover may have been sent home in between) runs only on a collision.
    if (e.xy[O1] == e.xy[I] || e.xy[O2] == e.xy[I]) {
        if (e.pac[I]) {
            if (!e.pac[O1] && e.xy[O1] == e.xy[I]) {
                if (e.scared[O1] <= 0) { kill_dump<I>(e, c, d_red, d_blue); send_home(e, c, I); }
                else send_home(e, c, O1);
            }
            if (!e.pac[O2] && e.xy[O2] == e.xy[I]) {
                if (e.scared[O2] <= 0) { kill_dump<I>(e, c, d_red, d_blue); send_home(e, c, I); }
                else send_home(e, c, O2);
            }
        } else {
            if (e.pac[O1] && e.xy[O1] == e.xy[I]) {
                if (e.scared[I] <= 0) { kill_dump<O1>(e, c, d_red, d_blue); send_home(e, c, O1); }
                else send_home(e, c, I);
            }
            if (e.pac[O2] && e.xy[O2] == e.xy[I]) {
                if (e.scared[I] <= 0) { kill_dump<O2>(e, c, d_red, d_blue); send_home(e, c, O2); }
                else send_home(e, c, I);
            }
        }
    }
    e.scared[I] = e.scared[I] > 1 ? e.scared[I] - 1 : 0;                  // capture.py:562-567, mover only
    e.score += sc;                                                        // capture.py:121
    return sc;
}

// agents/baselineTeam.py:65-187 evaluated in the kernel (action codes -3 offensive / -4 defensive, include/pmx.h): the
// successor of every legal action is generated for real (on a register copy of the agents and a scratch LDS copy of the
// food column), scored with the reference's features x weights, and one of the best actions is drawn with the
// counter-based generator; with no food left to eat the agent walks home (:81-90).
// The bots' draws (include/pmx.h): h(salt) = lowbias32(rng_key ^ ticks * 0x85EBCA77 ^ agent * 0xC2B2AE3D ^ salt); salt 0 is
// random_legal's draw.
#define PMX_SALT_BEST 0x5bd1e995u       // choice among the best actions
#define PMX_SALT_EXPLORE 0xA511E9B3u    // approxQTeam's epsilon test
#define PMX_BOT_HOME 1                  // flag bits returned beside the action (action | flags << 8)
#define PMX_BOT_EXPLORED 2
#define PMX_BOT_SEEN_LO 4               // sight form only: the lower-index / higher-index enemy is seen (bot_seen)
#define PMX_BOT_SEEN_HI 8
// (bot_hash, the generator itself, is in pmx_belief.h: the sonar's draw uses it too)
// floor(x * n / 2^32)-th set action of `mask` in the reference's list order N,S,E,W,Stop
__device__ __forceinline__ int pick_in_order(int mask, uint32_t x)
{
    int kk = (int)(((uint64_t)x * (uint32_t)__popc(mask)) >> 32);
    int pick = 4;
    const int order[5] = { 0, 2, 1, 3, 4 };
    for (int j = 0; j < 5; ++j) {
        const int a = order[j];
        if ((mask >> a) & 1) { if (kk == 0) pick = a; --kk; }
    }
    return pick;
}

// The walk home of the reflex bots (agents/baselineTeam.py:81-90, agents/approxQTeam.py:77-86 and :324-333): the real
// successor of every legal action in list order, first minimum of the maze distance from the start cell, no draw.
template <int I>
__device__ __noinline__ int bot_home_walk(const Env &e, const Ctx &c, int legal)
{
    const int start_idx = c.cidx[(c.start_xy[I] >> 8) * 32 + (c.start_xy[I] & 0xFF)];
    int home_best = 9999, home_act = -1;
    const int order[5] = { 0, 2, 1, 3, 4 };
    for (int k = 0; k < 5; ++k) {
        const int a = order[k];
        if (!((legal >> a) & 1)) continue;
        Env t = e;
        for (int y = 0; y < c.H; ++y) c.fd2[y * PMX_RULE_BLOCK] = c.fd[y * PMX_RULE_BLOCK];
        Ctx c2 = c;
        c2.fd = c.fd2;
        bool rl; int dr = 0, db = 0;
        substep_core<I>(t, c2, a, rl, dr, db);
        const int my = c.cidx[(t.xy[I] >> 8) * 32 + (t.xy[I] & 0xFF)];
        const int hd = c.dist[(size_t)start_idx * c.n_cells + my];
        if (hd < home_best) { home_best = hd; home_act = a; }
    }
    return home_act;
}

// home_at: the agent walks home when at most that many pellets are left to eat (baselineTeam 0; approxQTeam's defender 2,
// agents/approxQTeam.py:324).  vals (NULL inside a tick): receives the feature sum of every legal action, indexed by action
// code (pmx_bot_query); the evaluation then runs even when the agent walks home.  Returns action | flags << 8.
template <int I>
__device__ __noinline__ int bot_action(const Env &e, const Ctx &c, bool defensive, int home_at, double *vals)
{
    constexpr bool RED = (I % 2) == 0;
    constexpr int O1 = RED ? 1 : 0, O2 = O1 + 2;
    const int legal = legal_mask(c.wl, c.wls, (int)(e.xy[I] & 0xFF), (int)(e.xy[I] >> 8));
    const uint32_t enemy_mask = RED ? c.hi_mask : c.lo_mask;      // getFood: the other side's pellets
    int food_left = 0;
    for (int y = 0; y < c.H; ++y) food_left += __popc(c.fd[y * PMX_RULE_BLOCK] & enemy_mask);
    int home_act = -1;
    if (food_left <= home_at) {
        home_act = bot_home_walk<I>(e, c, legal) | (PMX_BOT_HOME << 8);
        if (!vals) return home_act;
    }
    int best = -(1 << 30), best_mask = 0;
    const int order[5] = { 0, 2, 1, 3, 4 };
    const int rev[5] = { 2, 3, 0, 1, 4 };
    for (int k = 0; k < 5; ++k) {
        const int a = order[k];
        if (!((legal >> a) & 1)) continue;
        Env t = e;
        for (int y = 0; y < c.H; ++y) c.fd2[y * PMX_RULE_BLOCK] = c.fd[y * PMX_RULE_BLOCK];
        Ctx c2 = c;
        c2.fd = c.fd2;
        bool rl; int dr = 0, db = 0;
        substep_core<I>(t, c2, a, rl, dr, db);
        const int my = c.cidx[(t.xy[I] >> 8) * 32 + (t.xy[I] & 0xFF)];
        const uint8_t *drow = c.dist + (size_t)my * c.n_cells;
        int val;
        if (!defensive) {
            int cnt = 0, mind = 1 << 30;
            for (int y = 0; y < c.H; ++y) {
                uint32_t m = c.fd2[y * PMX_RULE_BLOCK] & enemy_mask;
                cnt += __popc(m);
                while (m) {
                    const int x = __ffs(m) - 1;
                    m &= m - 1;
                    const int d = drow[c.cidx[y * 32 + x]];
                    mind = d < mind ? d : mind;
                }
            }
            val = -100 * cnt - (cnt > 0 ? mind : 0);
        } else {
            int num_inv = 0, mind = 1 << 30;
            if (t.pac[O1]) { ++num_inv; const int d = drow[c.cidx[(t.xy[O1] >> 8) * 32 + (t.xy[O1] & 0xFF)]]; mind = d < mind ? d : mind; }
            if (t.pac[O2]) { ++num_inv; const int d = drow[c.cidx[(t.xy[O2] >> 8) * 32 + (t.xy[O2] & 0xFF)]]; mind = d < mind ? d : mind; }
            val = -1000 * num_inv + 100 * (t.pac[I] ? 0 : 1) - (num_inv > 0 ? 10 * mind : 0) - (a == 4 ? 100 : 0) - (a == rev[e.dir[I]] ? 2 : 0);
        }
        if (val > best) { best = val; best_mask = 1 << a; }
        else if (val == best) best_mask |= 1 << a;
        if (vals) vals[a] = (double)val;
    }
    if (home_act >= 0) return home_act;
    return pick_in_order(best_mask, bot_hash(c.rng_key, e.ticks, I, PMX_SALT_BEST));
}

// bot_action under the sight rule (the handle has a bot sight, pmx_set_bot_sight).  It is bot_action's text once more and not a
// template both share: as a wrapper around a shared always-inlined body, bot_action<I> -- four calls per env and tick on every
// bots handle -- came out 16 .. 36 bytes shorter and differently scheduled (profiles/fog_bots/README.md).
// `seen` bit 0 / 1 = enemy O1 / O2 is within the sight range of the deciding agent or its mate IN THE STATE e; a defender counts an enemy as an invader of a successor only when that bit is set
// (agents/baselineTeam.py:174, agents/approxQTeam.py:394 filter on getPosition() != None, and GameState.makeObservation,
// capture.py:268-292, hides a far enemy once, before any successor is generated).  The successors themselves stay the full
// state's: a one-move successor can collide only with an enemy on the cell the mover reaches, that enemy is at Manhattan
// distance <= 1 from the mover before the move and hence seen for every sight range >= 1, so substep_core needs no
// checkDeath skip (capture.py:681, :707) -- which is why sight 0 is refused.  The offensive features read no enemy.
template <int I>
__device__ __noinline__ int bot_action_sight(const Env &e, const Ctx &c, bool defensive, int home_at, double *vals, int seen)
{
    constexpr bool RED = (I % 2) == 0;
    constexpr int O1 = RED ? 1 : 0, O2 = O1 + 2;
    const int legal = legal_mask(c.wl, c.wls, (int)(e.xy[I] & 0xFF), (int)(e.xy[I] >> 8));
    const uint32_t enemy_mask = RED ? c.hi_mask : c.lo_mask;      // getFood: the other side's pellets
    int food_left = 0;
    for (int y = 0; y < c.H; ++y) food_left += __popc(c.fd[y * PMX_RULE_BLOCK] & enemy_mask);
    int home_act = -1;
    if (food_left <= home_at) {
        home_act = bot_home_walk<I>(e, c, legal) | (PMX_BOT_HOME << 8);
        if (!vals) return home_act;
    }
    int best = -(1 << 30), best_mask = 0;
    const int order[5] = { 0, 2, 1, 3, 4 };
    const int rev[5] = { 2, 3, 0, 1, 4 };
    for (int k = 0; k < 5; ++k) {
        const int a = order[k];
        if (!((legal >> a) & 1)) continue;
        Env t = e;
        for (int y = 0; y < c.H; ++y) c.fd2[y * PMX_RULE_BLOCK] = c.fd[y * PMX_RULE_BLOCK];
        Ctx c2 = c;
        c2.fd = c.fd2;
        bool rl; int dr = 0, db = 0;
        substep_core<I>(t, c2, a, rl, dr, db);
        const int my = c.cidx[(t.xy[I] >> 8) * 32 + (t.xy[I] & 0xFF)];
        const uint8_t *drow = c.dist + (size_t)my * c.n_cells;
        int val;
        if (!defensive) {
            int cnt = 0, mind = 1 << 30;
            for (int y = 0; y < c.H; ++y) {
                uint32_t m = c.fd2[y * PMX_RULE_BLOCK] & enemy_mask;
                cnt += __popc(m);
                while (m) {
                    const int x = __ffs(m) - 1;
                    m &= m - 1;
                    const int d = drow[c.cidx[y * 32 + x]];
                    mind = d < mind ? d : mind;
                }
            }
            val = -100 * cnt - (cnt > 0 ? mind : 0);
        } else {
            int num_inv = 0, mind = 1 << 30;
            if (t.pac[O1] && (seen & 1)) { ++num_inv; const int d = drow[c.cidx[(t.xy[O1] >> 8) * 32 + (t.xy[O1] & 0xFF)]]; mind = d < mind ? d : mind; }
            if (t.pac[O2] && (seen & 2)) { ++num_inv; const int d = drow[c.cidx[(t.xy[O2] >> 8) * 32 + (t.xy[O2] & 0xFF)]]; mind = d < mind ? d : mind; }
            val = -1000 * num_inv + 100 * (t.pac[I] ? 0 : 1) - (num_inv > 0 ? 10 * mind : 0) - (a == 4 ? 100 : 0) - (a == rev[e.dir[I]] ? 2 : 0);
        }
        if (val > best) { best = val; best_mask = 1 << a; }
        else if (val == best) best_mask |= 1 << a;
        if (vals) vals[a] = (double)val;
    }
    if (home_act >= 0) return home_act;
    return pick_in_order(best_mask, bot_hash(c.rng_key, e.ticks, I, PMX_SALT_BEST));
}

// agents/approxQTeam.py:49-110, 194-292 ApproxQLearningOffense evaluated in the kernel (action code -5): a linear Q function
// of (state, action) with the team file's fixed weights, epsilon-greedy with epsilon 0.1, no learning.  Nothing is generated:
// the features read the agent's cell plus the action vector.  The Q value is summed in float64 in the insertion order of the
// reference's feature dictionary (bias, ghosts one step away, eats-food, closest-food), every product and sum rounded on its
// own, so that it equals the reference's Python float bit for bit.  Three draws (include/pmx.h): explore iff
// h(PMX_SALT_EXPLORE) < ceil(2^32 / 10); exploring plays random_legal's action; otherwise the best set is drawn from as
// bot_action draws.  With at most two pellets left the agent walks home (:77-86).  Returns action | flags << 8.
// SIGHT: a ghost is counted only when its `seen` bit is set (agents/approxQTeam.py:230 filters on getPosition() != None); at
// a sight range >= 2 a ghost within one step of the next cell is always seen, so the rule bites at sight 1 only.
template <int I, bool SIGHT>
__device__ __forceinline__ int approxq_action_impl(const Env &e, const Ctx &c, double *vals, int seen)
{
    constexpr bool RED = (I % 2) == 0;
    constexpr int O1 = RED ? 1 : 0, O2 = O1 + 2;
    const int px = (int)(e.xy[I] & 0xFF), py = (int)(e.xy[I] >> 8);
    const int legal = legal_mask(c.wl, c.wls, px, py);
    const uint32_t enemy_mask = RED ? c.hi_mask : c.lo_mask;      // getFood: the other side's pellets
    int food_left = 0;
    for (int y = 0; y < c.H; ++y) food_left += __popc(c.fd[y * PMX_RULE_BLOCK] & enemy_mask);
    int home_act = -1;
    if (food_left <= 2) {
        home_act = bot_home_walk<I>(e, c, legal) | (PMX_BOT_HOME << 8);
        if (!vals) return home_act;
    }
    const double w_bias = -9.280875042529367, w_ghosts = -16.6612110039328, w_eats = 11.127808437648863,
                 w_closest = -3.099192562140742;                  // agents/approxQTeam.py:58-61
    const double tenth = __ddiv_rn(1.0, 10.0), cells = (double)(c.W * c.H);
    double best = 0.0;
    int best_mask = 0;
    const int order[5] = { 0, 2, 1, 3, 4 };
#pragma unroll 1
    for (int k = 0; k < 5; ++k) {
        const int a = order[k];
        if (!((legal >> a) & 1)) continue;
        const int nx = px + (a == 1) - (a == 3), ny = py + (a == 0) - (a == 2);
        // ghosts one step away: opponents that are not Pacman (scared or not) on the cell or next to it (Actions.getLegalNeighbors
        // of the ghost's cell includes the cell itself; the next cell is open, so no wall test is left)
        int g = 0;
        if (!e.pac[O1] && (!SIGHT || (seen & 1))) g += (abs((int)(e.xy[O1] & 0xFF) - nx) + abs((int)(e.xy[O1] >> 8) - ny)) <= 1;
        if (!e.pac[O2] && (!SIGHT || (seen & 2))) g += (abs((int)(e.xy[O2] & 0xFF) - nx) + abs((int)(e.xy[O2] >> 8) - ny)) <= 1;
        const bool eats = g == 0 && (((c.fd[ny * PMX_RULE_BLOCK] & enemy_mask) >> nx) & 1u);
        // closestFood's breadth-first search = the smallest entry of the next cell's row of the distance matrix
        const uint8_t *drow = c.dist + (size_t)c.cidx[ny * 32 + nx] * c.n_cells;
        int mind = 255;
        for (int y = 0; y < c.H; ++y) {
            uint32_t m = c.fd[y * PMX_RULE_BLOCK] & enemy_mask;
            while (m) {
                const int x = __ffs(m) - 1;
                m &= m - 1;
                const int d = drow[c.cidx[y * 32 + x]];
                mind = d < mind ? d : mind;
            }
        }
        double q = 0.0;
        q = __dadd_rn(q, __dmul_rn(tenth, w_bias));
        q = __dadd_rn(q, __dmul_rn(__ddiv_rn((double)g, 10.0), w_ghosts));
        if (eats) q = __dadd_rn(q, __dmul_rn(tenth, w_eats));
        if (mind != 255) q = __dadd_rn(q, __dmul_rn(__ddiv_rn(__ddiv_rn((double)mind, cells), 10.0), w_closest));
        if (best_mask == 0 || q > best) { best = q; best_mask = 1 << a; }
        else if (q == best) best_mask |= 1 << a;
        if (vals) vals[a] = q;
    }
    if (home_act >= 0) return home_act;
    if (bot_hash(c.rng_key, e.ticks, I, PMX_SALT_EXPLORE) < 0x1999999Au)
        return random_legal(legal, c.rng_key, e.ticks, I) | (PMX_BOT_EXPLORED << 8);
    return pick_in_order(best_mask, bot_hash(c.rng_key, e.ticks, I, PMX_SALT_BEST));
}
template <int I>
__device__ __noinline__ int approxq_action(const Env &e, const Ctx &c, double *vals)
{
    return approxq_action_impl<I, false>(e, c, vals, 3);
}
template <int I>
__device__ __noinline__ int approxq_action_sight(const Env &e, const Ctx &c, double *vals, int seen)
{
    return approxq_action_impl<I, true>(e, c, vals, seen);
}

// The contest's sight rule for bot agent I (GameState.makeObservation, capture.py:268-292): enemy O is seen iff it is within
// `sight` Manhattan cells of I or of I's mate.  Bit 0: enemy O1 (the lower index), bit 1: enemy O2.  Four distances on the
// state the decision starts from, in registers; a hidden enemy stays hidden in every successor of that decision.
template <int I>
__device__ __forceinline__ int bot_seen(const Env &e, int sight)
{
    constexpr int O1 = (I % 2) == 0 ? 1 : 0, O2 = O1 + 2, M = (I + 2) % 4;
    const int xi = (int)(e.xy[I] & 0xFF), yi = (int)(e.xy[I] >> 8), xm = (int)(e.xy[M] & 0xFF), ym = (int)(e.xy[M] >> 8);
    const int x1 = (int)(e.xy[O1] & 0xFF), y1 = (int)(e.xy[O1] >> 8), x2 = (int)(e.xy[O2] & 0xFF), y2 = (int)(e.xy[O2] >> 8);
    const int d1 = min(abs(x1 - xi) + abs(y1 - yi), abs(x1 - xm) + abs(y1 - ym));
    const int d2 = min(abs(x2 - xi) + abs(y2 - yi), abs(x2 - xm) + abs(y2 - ym));
    return (int)(d1 <= sight) | ((int)(d2 <= sight) << 1);
}

// what bot `code` (-2 .. -6) plays for agent I in state e, as action | flags << 8; the tick (vals NULL) and pmx_bot_query go
// through this one function.  SIGHT: the sight form, which also reports the two seen bits as flags PMX_BOT_SEEN_LO / _HI.
template <int I, bool SIGHT = false>
__device__ __forceinline__ int bot_decide(const Env &e, const Ctx &c, int code, double *vals, int sight = 0)
{
    if constexpr (SIGHT) {
        const int seen = bot_seen<I>(e, sight);
        int r;
        if (code == -5) r = approxq_action_sight<I>(e, c, vals, seen);
        else if (code == -3) r = bot_action<I>(e, c, false, 0, vals);
        else r = bot_action_sight<I>(e, c, true, code == -6 ? 2 : 0, vals, seen);
        return r | (seen << 10);
    }
    if (code == -5) return approxq_action<I>(e, c, vals);
    if (code == -3) return bot_action<I>(e, c, false, 0, vals);
    return bot_action<I>(e, c, true, code == -6 ? 2 : 0, vals);
}

// BOTS: the handle was created with pmx_config.enable_bots; only that kernel variant carries the bot code (action codes
// -3 .. -6; it costs registers and a stack frame for the agent state: +3 us per tick on 16 k envs even when no bot code is used)
// BOTS == 2: the bots variant with the sight rule (PmxTickParams::bot_sight, a separate instantiation of every kernel that
// carries bot code, so that handles without a sight run the code they ran before)
template <int I, int BOTS>
__device__ __forceinline__ int substep(Env &e, const Ctx &c, int action, bool &req_legal, int &d_red, int &d_blue, int sight = 0)
{
    if (action == -2) action = random_legal(legal_mask(c.wl, c.wls, (int)(e.xy[I] & 0xFF), (int)(e.xy[I] >> 8)), c.rng_key, e.ticks, I);
    if constexpr (BOTS) {
        if (action <= -3 && action >= -6 && c.dist) action = bot_decide<I, BOTS == 2>(e, c, action, nullptr, sight) & 0xFF;
    }
    return substep_core<I>(e, c, action, req_legal, d_red, d_blue);
}

// One iteration of the loop gymPacMan.py:149-169 for agent I: shaped reward (from the successor, which is what the
// reference's shadow successor equals) + the transition itself.
template <int I, int BOTS>
__device__ __forceinline__ void tick_substep(Env &e, Acc &a, const Ctx &c, int action, int sight = 0)
{
    constexpr bool RED = (I % 2) == 0;
    constexpr int O1 = RED ? 1 : 0, O2 = O1 + 2;
    const int pac1 = e.pac[O1], pac2 = e.pac[O2];
    bool req_legal;
    int d_red = 0, d_blue = 0;
    const int sc = substep<I, BOTS>(e, c, action, req_legal, d_red, d_blue, sight);
    double r = RED ? a.red_r : a.blue_r;
    if (RED) {                                                            // gymPacMan.py:233-242
        if (d_red > 0) r += 1.0;
        if (d_blue < 0) r += 0.1;
    } else {                                                              // :244-253
        if (d_blue > 0) r += 1.0;
        if (d_red < 0) r += 0.1;
    }
    if (c.defence_reward) {
        if (pac1 && !e.pac[O1] && e.xy[O1] == c.start_xy[O1]) r += 0.25;
        if (pac2 && !e.pac[O2] && e.xy[O2] == c.start_xy[O2]) r += 0.25;
    }
    if (c.legal_reward && req_legal) r += 0.01;                           // :254-257
    if (RED) { a.red_r = r; a.red_sc += sc; } else { a.blue_r = r; a.blue_sc -= sc; }
    a.n_red += d_red; a.n_blue += d_blue;
    a.sc_total += sc;                                                     // :153-162
    e.self_after[I] = e.xy[I] | ((uint32_t)e.carry[I] << 16);
}

// HB > 0: the board has at most HB rows and the row loops are fully unrolled with predicated accesses, so that all HBM
// loads (or all LDS reads) of a state are in flight at once.  With a run-time trip count the compiler emits
// load -> s_waitcnt -> ds_write per row: H dependent memory round trips on a kernel that runs one wave per SIMD.
// The run-time loops remain for the per-agent and query kernels, which are not on the hot path.
struct RawEnv {            // the non-row state words as loaded, before unpacking
    uint32_t a[4], b[4], capw[2], score, steps, ticks;
};
// phase 1 of the hot-path load: nothing but global loads (needs only the kernel arguments), issued before the layout
// set-up so that the HBM latency overlaps it
template <int HB>
__device__ __forceinline__ void load_env_issue(RawEnv &r, uint32_t (&rows)[HB], const uint32_t *st, int N, int env, int H)
{
#pragma unroll
    for (int y = 0; y < HB; ++y) rows[y] = y < H ? st[(size_t)y * N + env] : 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r.a[i] = st[(size_t)PMX_W_AGENT_A(H, i) * N + env];
        r.b[i] = st[(size_t)PMX_W_AGENT_B(H, i) * N + env];
    }
    r.capw[0] = st[(size_t)PMX_W_CAPS(H, 0) * N + env];
    r.capw[1] = st[(size_t)PMX_W_CAPS(H, 1) * N + env];
    r.score = st[(size_t)PMX_W_SCORE(H) * N + env];
    r.steps = st[(size_t)PMX_W_STEPS(H) * N + env];
    r.ticks = st[(size_t)PMX_W_TICKS(H) * N + env];
}
// phase 2: unpack into registers, food rows into this lane's LDS column
template <int HB>
__device__ __forceinline__ void load_env_commit(Env &e, const Ctx &c, const RawEnv &r, const uint32_t (&rows)[HB])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) { unpack_a(e, i, r.a[i]); unpack_b(e, i, r.b[i]); }
    e.capw[0] = r.capw[0]; e.capw[1] = r.capw[1];
    e.score = (int)r.score; e.steps = (int)r.steps; e.ticks = r.ticks;
#pragma unroll
    for (int y = 0; y < HB; ++y)
        if (y < c.H) c.fd[y * PMX_RULE_BLOCK] = rows[y];
}
// capture.py:332-342 halfGrid sums of the state as loaded (the rows are still in registers: no LDS round trip)
template <int HB>
__device__ __forceinline__ void count_food(Acc &a, const Ctx &c, const uint32_t (&rows)[HB])
{
    int nr = 0, nb = 0;
#pragma unroll
    for (int y = 0; y < HB; ++y) { nr += __popc(rows[y] & c.lo_mask); nb += __popc(rows[y] & c.hi_mask); }
    a.n_red = nr; a.n_blue = nb;
}

__device__ __forceinline__ void load_env(Env &e, const Ctx &c, const uint32_t *st, int N, int env)
{
    for (int y = 0; y < c.H; ++y) c.fd[y * PMX_RULE_BLOCK] = st[(size_t)y * N + env];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unpack_a(e, i, st[(size_t)PMX_W_AGENT_A(c.H, i) * N + env]);
        unpack_b(e, i, st[(size_t)PMX_W_AGENT_B(c.H, i) * N + env]);
    }
    e.capw[0] = st[(size_t)PMX_W_CAPS(c.H, 0) * N + env];
    e.capw[1] = st[(size_t)PMX_W_CAPS(c.H, 1) * N + env];
    e.score = (int)st[(size_t)PMX_W_SCORE(c.H) * N + env];
    e.steps = (int)st[(size_t)PMX_W_STEPS(c.H) * N + env];
    e.ticks = st[(size_t)PMX_W_TICKS(c.H) * N + env];
}
template <int HB = 0>
__device__ __forceinline__ void store_snapshot(const Env &e, const Ctx &c, uint32_t *st, int N, int env)
{
    if constexpr (HB > 0) {
        uint32_t rows[HB];
#pragma unroll
        for (int y = 0; y < HB; ++y) rows[y] = y < c.H ? c.fd[y * PMX_RULE_BLOCK] : 0u;
#pragma unroll
        for (int y = 0; y < HB; ++y)
            if (y < c.H) st[(size_t)y * N + env] = rows[y];
    } else {
        for (int y = 0; y < c.H; ++y) st[(size_t)y * N + env] = c.fd[y * PMX_RULE_BLOCK];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        st[(size_t)PMX_W_AGENT_A(c.H, i) * N + env] = pack_a(e, i);
        st[(size_t)PMX_W_AGENT_B(c.H, i) * N + env] = pack_b(e, i);
    }
    st[(size_t)PMX_W_CAPS(c.H, 0) * N + env] = e.capw[0];
    st[(size_t)PMX_W_CAPS(c.H, 1) * N + env] = e.capw[1];
}
// The same words with 16-byte stores: a dword store per word and lane is 22 (snapshot) or 25 (state) store instructions of
// 256 bytes each, and on a kernel that runs ONE wave per CU their issue time is on the critical path (shader clock: a sub-step
// with its snapshot took 2 250-2 700 ticks, one without 1 200).  The SoA rows of 64 consecutive envs are 256 contiguous
// bytes, and the food rows already sit in LDS as [row][lane]: lane L of instruction k reads row 4k + (L >> 4), envs
// 4 (L & 15) .. + 3 with one ds_read_b128 and stores them with one global_store_dwordx4 -- 3 + 3 instructions per snapshot
// instead of 22.  The non-row words go through an LDS staging block in the same shape.  Needs all 64 lanes live
// (N % 64 == 0), which the caller checks; LDS operations of one wave execute in order, so later row updates cannot overtake.
// rows 4k + sub (k = K0 .. K1 - 1) of an LDS block [row][lane] -> SoA words (word0 + row) of 64 envs, 16 bytes per lane
template <int K0, int K1>
__device__ __forceinline__ void wide_group(const uint32_t *lds_rows, int n_rows, int word0, int sub, int q4, uint32_t *dst, int N)
{
    if constexpr (K0 < K1) {
        const int r = 4 * K0 + sub;
        const uint4 v = *reinterpret_cast<const uint4 *>(lds_rows + (r < n_rows ? r : 0) * PMX_RULE_BLOCK + q4);
        wide_group<K0 + 1, K1>(lds_rows, n_rows, word0, sub, q4, dst, N);       // the later reads are issued before this store
        if (r < n_rows) *reinterpret_cast<uint4 *>(dst + (size_t)(word0 + r) * N) = v;
    }
}
template <int HB, int NW>
__device__ __forceinline__ void store_words_wide(const Ctx &c, const uint32_t (&w)[NW], uint32_t *st, int N)
{
    const int lane = threadIdx.x, sub = lane >> 4, q4 = 4 * (lane & 15);
    uint32_t *dst = st + (size_t)blockIdx.x * PMX_RULE_BLOCK + q4;
#pragma unroll
    for (int i = 0; i < NW; ++i) c.stg[i * PMX_RULE_BLOCK + lane] = w[i];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // (reads unconditional, with the row clamped, and no register ARRAY of them: an array the compiler cannot fully scalarise
    // goes to scratch memory, and a scratch reload waits for vmcnt(0), i.e. for every store in flight)
    constexpr int KR = HB / 4, KW = (NW + 3) / 4;
    wide_group<0, KR>(c.rows0, c.H, 0, sub, q4, dst, N);
    wide_group<0, KW>(c.stg, NW, c.H, sub, q4, dst, N);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");          // the staging block is rewritten by the next call
    __builtin_amdgcn_wave_barrier();
}
template <int HB>
__device__ __forceinline__ void store_snapshot_wide(const Env &e, const Ctx &c, uint32_t *st, int N)
{
    uint32_t w[10];
#pragma unroll
    for (int i = 0; i < 4; ++i) { w[i] = pack_a(e, i); w[4 + i] = pack_b(e, i); }
    w[8] = e.capw[0]; w[9] = e.capw[1];
    store_words_wide<HB, 10>(c, w, st, N);
}
template <int HB>
__device__ __forceinline__ void store_env_wide(const Env &e, const Ctx &c, uint32_t *st, int N)
{
    uint32_t w[13];
#pragma unroll
    for (int i = 0; i < 4; ++i) { w[i] = pack_a(e, i); w[4 + i] = pack_b(e, i); }
    w[8] = e.capw[0]; w[9] = e.capw[1];
    w[10] = (uint32_t)e.score; w[11] = (uint32_t)e.steps; w[12] = e.ticks;
    store_words_wide<HB, 13>(c, w, st, N);
}
template <int HB = 0>
__device__ __forceinline__ void store_env(const Env &e, const Ctx &c, uint32_t *st, int N, int env)
{
    store_snapshot<HB>(e, c, st, N, env);
    st[(size_t)PMX_W_SCORE(c.H) * N + env] = (uint32_t)e.score;
    st[(size_t)PMX_W_STEPS(c.H) * N + env] = (uint32_t)e.steps;
    st[(size_t)PMX_W_TICKS(c.H) * N + env] = e.ticks;
}
// random_layout=True (gymPacMan.py:98-100): the layout an env moves to when it is reset; counter-based draw keyed by
// (seed, env, the env's tick counter) -- a build-side definition, include/pmx.h redraw_layouts
__device__ __forceinline__ int redraw_layout(uint32_t key, uint32_t ticks, int n_layouts)
{
    uint32_t x = key ^ (ticks * 0x85EBCA77u) ^ 0x4C41594Fu;
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return (int)(((uint64_t)x * (uint32_t)n_layouts) >> 32);
}

// point the lane's context at another layout of the pool: layout record, start cells, and the lane's wall column in LDS
__device__ __forceinline__ void switch_layout(Ctx &c, const PmxTickParams &p, int env, int li)
{
    p.layout_idx_rw[env] = li;
    c.L = p.lay + li;
#pragma unroll
    for (int i = 0; i < 4; ++i) c.start_xy[i] = (uint32_t)c.L->startx[i] | ((uint32_t)c.L->starty[i] << 8);
    uint32_t *w = const_cast<uint32_t *>(c.wl);
    for (int y = 0; y < 32; ++y) w[y * c.wls] = y < c.H ? c.L->walls[y] : 0xFFFFFFFFu;
}

__device__ __forceinline__ void init_env(Env &e, const Ctx &c)
{
    for (int y = 0; y < c.H; ++y) c.fd[y * PMX_RULE_BLOCK] = c.L->food0[y];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        e.xy[i] = c.start_xy[i]; e.dir[i] = 4;
        e.pac[i] = 0; e.scared[i] = 0; e.carry[i] = 0; e.ret[i] = 0;
    }
    e.capw[0] = c.L->capw0[0]; e.capw[1] = c.L->capw0[1];
    e.score = 0; e.steps = 0;
}

// gymPacMan.py:171-193: everything after the four sub-steps.
// Returns true when the env finished and was reset to the fresh game (auto_reset).
// FRESH_SNAP = false (pmx_tick_fused_kernel): the caller stores the fresh game's snapshots itself.
template <int HB = 0, bool FRESH_SNAP = true>
__device__ __forceinline__ bool tick_finish(Env &e, Acc &a, const Ctx &c_in, const PmxTickParams &p, int env, bool fused)
{
    Ctx c = c_in;             // a reset may move the env to another layout of the pool (redraw_layouts)
    double blue_r = a.blue_r + (double)(a.blue_sc > 0 ? a.blue_sc : 0);   // :171-172
    double red_r = a.red_r + (double)(a.red_sc > 0 ? a.red_sc : 0);
    int n_red = 0, n_blue = 0;                                            // capture.py:332-342 halfGrid sums
    if constexpr (HB > 0) {
        n_red = a.n_red; n_blue = a.n_blue;      // counted when the state was loaded, updated by every eaten / dumped pellet
    } else {
        for (int y = 0; y < c.H; ++y) {
            uint32_t row = c.fd[y * PMX_RULE_BLOCK];
            n_red += __popc(row & c.lo_mask);
            n_blue += __popc(row & c.hi_mask);
        }
    }
    bool done = (n_blue == 0 && e.carry[0] == 0 && e.carry[2] == 0) ||    // gymPacMan.py:261-270
                (n_red == 0 && e.carry[1] == 0 && e.carry[3] == 0) || (e.steps >= p.length);
    if (done) {                                                           // :177-182
        const int fs = e.score;
        if (fs < 0) blue_r += 20.0 + (1.0 / 5) * (double)(-fs);
        else if (fs > 0) red_r += 20.0 + (1.0 / 5) * (double)fs;
    }
    e.steps += 1;                                                         // :189
    e.ticks += 1;
    if (p.agent_out && fused) {
        uint4 v = make_uint4(e.self_after[0], e.self_after[1], e.self_after[2], e.self_after[3]);
        reinterpret_cast<uint4 *>(p.agent_out)[env] = v;
    }
    if (p.reward) { p.reward[2 * (size_t)env] = red_r; p.reward[2 * (size_t)env + 1] = blue_r; }
    if (p.done) p.done[env] = (uint8_t)done;
    if (p.score_change) p.score_change[env] = a.sc_total;
    if (p.score) p.score[env] = e.score;
    if (done && p.auto_reset) {
        if (p.layout_idx_rw) switch_layout(c, p, env, redraw_layout(c.rng_key, e.ticks, p.n_layouts));
        init_env(e, c);
        // the observations of a finished env are those of the fresh game for all four agents (gymPacMan.py:135-137)
        if constexpr (FRESH_SNAP) {
            const size_t snap_sz = (size_t)PMX_SNAP_WORDS(c.H) * p.N;
            for (int s = 0; s < 3; ++s) store_snapshot(e, c, p.snap + s * snap_sz, p.N, env);
        }
    }
    if (p.legal) {
        uint32_t m = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) m |= (uint32_t)legal_mask(c.wl, c.wls, (int)(e.xy[i] & 0xFF), (int)(e.xy[i] >> 8)) << (8 * i);
        reinterpret_cast<uint32_t *>(p.legal)[env] = m;
    }
    return done && p.auto_reset;
}

// env0 = the env of this lane, tid = its lane in the rule wave.  The caller makes the LDS writes visible to the wave(s) that
// read them: make_ctx with a block barrier, pmx_tick_fused_kernel (whose rule wave is one of sixteen) with a wave barrier.
__device__ __forceinline__ Ctx make_ctx_fill(const PmxTickParams &p, uint32_t *lds, const int env0, const unsigned tid)
{
    Ctx c;
    const bool multi = p.layout_idx != nullptr;
    c.L = p.lay + ((multi && env0 < p.N) ? p.layout_idx[env0] : 0);
    c.W = p.lay_W; c.H = p.lay_H; c.half = p.lay_half; c.n_dump = p.lay_n_dump;       // identical in every layout of a handle
    c.dump = p.dump;
    c.legal_reward = p.legal_reward; c.defence_reward = p.defence_reward;
    c.wl = multi ? lds + 32 + PMX_MAX_H_LDS * PMX_RULE_BLOCK + tid : lds;
    c.wls = multi ? PMX_RULE_BLOCK : 1;
    c.fd = lds + 32 + tid;
    c.rows0 = lds + 32;
    c.stg = lds + 32 + (multi ? (3 * PMX_MAX_H_LDS + 32) : 3 * c.H) * PMX_RULE_BLOCK;
    c.fd2 = multi ? lds + 32 + 2 * PMX_MAX_H_LDS * PMX_RULE_BLOCK + tid : lds + 32 + c.H * PMX_RULE_BLOCK + tid;
    c.fd3 = multi ? lds + 32 + 3 * PMX_MAX_H_LDS * PMX_RULE_BLOCK + tid : lds + 32 + 2 * c.H * PMX_RULE_BLOCK + tid;
    c.dist = p.dist ? p.dist + c.L->dist_off : nullptr;
    c.cidx = p.cell_index ? p.cell_index + (size_t)(c.L - p.lay) * 1024 : nullptr;
    c.n_cells = c.L->n_cells;
    c.lo_mask = p.lo_mask; c.hi_mask = p.hi_mask;
#pragma unroll
    for (int i = 0; i < 4; ++i) c.start_xy[i] = (uint32_t)c.L->startx[i] | ((uint32_t)c.L->starty[i] << 8);
    c.rng_key = p.seed ^ ((uint32_t)env0 * 0x9E3779B1u);
    if (tid < 32) lds[tid] = tid < (unsigned)c.H ? p.lay->walls[tid] : 0xFFFFFFFFu;
    if (multi) {   // per-env layouts: every lane keeps its own wall column next to its food column
        uint32_t *w = lds + 32 + PMX_MAX_H_LDS * PMX_RULE_BLOCK + tid;
        uint32_t wr[32];
#pragma unroll
        for (int y = 0; y < 32; ++y) wr[y] = y < c.H ? c.L->walls[y] : 0xFFFFFFFFu;     // all loads in flight, then the LDS writes
#pragma unroll
        for (int y = 0; y < 32; ++y) w[y * PMX_RULE_BLOCK] = wr[y];
    }
    return c;
}

__device__ __forceinline__ Ctx make_ctx(const PmxTickParams &p, uint32_t *lds)
{
    Ctx c = make_ctx_fill(p, lds, blockIdx.x * PMX_RULE_BLOCK + threadIdx.x, threadIdx.x);
    __syncthreads();
    return c;
}

}  // namespace

__device__ __forceinline__ void write_walls(const PmxTickParams &p);    // defined with the observation kernels below

// dynamic LDS: 32 wall rows + 3 x H rows x PMX_RULE_BLOCK lanes (food, bots' scratch copy, dump_food's blocked-cell rows)
// Blocks rule_blocks .. gridDim.x - 1 (present when pmx_step splits the observation, see pmx_launch_rule) do not run the rules:
// they store the wall plane of the observation, the only plane bytes that do not depend on this tick's rules, while the rule
// blocks wait on their state loads and HBM would otherwise idle.  The branch is block-uniform; no block waits for another.
// The body is a macro, not a function the two kernels share: behind a function (by reference or by value, always inlined) the
// compiler schedules the eight existing instantiations differently (same registers, 40 .. 160 bytes more code each,
// profiles/fog_bots/README.md); as text in the kernel they keep their instruction streams.
// BOTS: 0 no bot code, 1 the bots variant, 2 the bots variant under the sight rule (p.bot_sight).
#define PMX_RULE_KERNEL_BODY(BOTS)                                                                                                  \
    extern __shared__ uint32_t lds[];                                                                                               \
    if ((int)blockIdx.x >= p.rule_blocks) {                                                                                         \
        write_walls(p);                                                                                                             \
        return;                                                                                                                     \
    }                                                                                                                               \
    const int env = blockIdx.x * PMX_RULE_BLOCK + threadIdx.x;                                                                      \
    const bool live = env < p.N;                                                                                                    \
    RawEnv raw;                                                                                                                     \
    uint32_t rows[HB];                                                                                                              \
    uint32_t av = 0;                                                                                                                \
    if (live) {                                                                                                                     \
        load_env_issue<HB>(raw, rows, p.state, p.N, env, p.lay_H);                                                                  \
        av = reinterpret_cast<const uint32_t *>(p.actions)[env];   /* 4 int8 actions */                                             \
    }                                                                                                                               \
    Ctx c = make_ctx(p, lds);                                                                                                       \
    if (!live) return;                                                                                                              \
    Env e;                                                                                                                          \
    load_env_commit<HB>(e, c, raw, rows);                                                                                           \
    Acc a = { 0.0, 0.0, 0, 0, 0, 0, 0 };                                                                                            \
    count_food<HB>(a, c, rows);                                                                                                     \
    const size_t snap_sz = (size_t)PMX_SNAP_WORDS(c.H) * p.N;                                                                       \
    const bool wide = (p.N & (PMX_RULE_BLOCK - 1)) == 0;   /* every wave is full: the 16-byte store path (store_words_wide) */      \
    tick_substep<0, BOTS>(e, a, c, (int)(int8_t)(av & 0xFF), p.bot_sight);                                                          \
    if (wide) store_snapshot_wide<HB>(e, c, p.snap, p.N); else store_snapshot<HB>(e, c, p.snap, p.N, env);                          \
    tick_substep<1, BOTS>(e, a, c, (int)(int8_t)((av >> 8) & 0xFF), p.bot_sight);                                                   \
    if (wide) store_snapshot_wide<HB>(e, c, p.snap + snap_sz, p.N); else store_snapshot<HB>(e, c, p.snap + snap_sz, p.N, env);      \
    tick_substep<2, BOTS>(e, a, c, (int)(int8_t)((av >> 16) & 0xFF), p.bot_sight);                                                  \
    if (wide) store_snapshot_wide<HB>(e, c, p.snap + 2 * snap_sz, p.N); else store_snapshot<HB>(e, c, p.snap + 2 * snap_sz, p.N, env); \
    tick_substep<3, BOTS>(e, a, c, (int)(int8_t)((av >> 24) & 0xFF), p.bot_sight);                                                  \
    tick_finish<HB>(e, a, c, p, env, true);                                                                                         \
    if (wide) store_env_wide<HB>(e, c, p.state, p.N); else store_env<HB>(e, c, p.state, p.N, env);

template <bool BOTS, int HB>
__global__ __launch_bounds__(PMX_RULE_BLOCK) void pmx_rule_kernel(PmxTickParams p)
{
    PMX_RULE_KERNEL_BODY(BOTS ? 1 : 0)
}
// the bots variant under the sight rule (handles with pmx_set_bot_sight)
template <int HB>
__global__ __launch_bounds__(PMX_RULE_BLOCK) void pmx_rule_sight_kernel(PmxTickParams p)
{
    PMX_RULE_KERNEL_BODY(2)
}

// pmx_step_agent: one sub-step; the accumulators of the open tick travel through the state words.
template <int I, int BOTS>
__device__ __forceinline__ void rule_agent_body(const PmxTickParams &p, uint32_t *lds)
{
    Ctx c = make_ctx(p, lds);
    const int env = blockIdx.x * PMX_RULE_BLOCK + threadIdx.x;
    if (env >= p.N) return;
    Env e;
    load_env(e, c, p.state, p.N, env);
    Acc a = { 0.0, 0.0, 0, 0, 0, 0, 0 };
    uint32_t *acc = p.state + (size_t)PMX_W_ACC(c.H) * p.N + env;
    if (I > 0) {
        a.red_r = __hiloint2double((int)acc[(size_t)1 * p.N], (int)acc[0]);
        a.blue_r = __hiloint2double((int)acc[(size_t)3 * p.N], (int)acc[(size_t)2 * p.N]);
        a.red_sc = (int)acc[(size_t)4 * p.N]; a.blue_sc = (int)acc[(size_t)5 * p.N]; a.sc_total = (int)acc[(size_t)6 * p.N];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)   // sub-steps not yet taken report the current state
        e.self_after[i] = e.xy[i] | ((uint32_t)e.carry[i] << 16);
    tick_substep<I, BOTS>(e, a, c, (int)p.actions[env], p.bot_sight);
    if (p.agent_out) p.agent_out[4 * (size_t)env + I] = e.self_after[I];
    if (I == 3) {
        tick_finish(e, a, c, p, env, false);
    } else {
        acc[0] = (uint32_t)__double2loint(a.red_r); acc[(size_t)1 * p.N] = (uint32_t)__double2hiint(a.red_r);
        acc[(size_t)2 * p.N] = (uint32_t)__double2loint(a.blue_r); acc[(size_t)3 * p.N] = (uint32_t)__double2hiint(a.blue_r);
        acc[(size_t)4 * p.N] = (uint32_t)a.red_sc; acc[(size_t)5 * p.N] = (uint32_t)a.blue_sc; acc[(size_t)6 * p.N] = (uint32_t)a.sc_total;
    }
    store_env(e, c, p.state, p.N, env);
}

// GameState.generateSuccessor as a stand-alone query (pmx_successor)
template <int I>
__device__ __forceinline__ void successor_body(const PmxTickParams &p, uint32_t *lds)
{
    Ctx c = make_ctx(p, lds);
    const int env = blockIdx.x * PMX_RULE_BLOCK + threadIdx.x;
    if (env >= p.N) return;
    Env e;
    load_env(e, c, p.state, p.N, env);
    bool req_legal;
    int d_red = 0, d_blue = 0;
    const int sc = substep<I, false>(e, c, (int)p.actions[env], req_legal, d_red, d_blue);
    if (p.score_change) p.score_change[env] = sc;
    store_env(e, c, p.state, p.N, env);
}

extern "C" __global__ __launch_bounds__(PMX_RULE_BLOCK) void pmx_successor_kernel(PmxTickParams p, int agent)
{
    extern __shared__ uint32_t lds[];
    switch (agent) {   // wave-uniform
    case 0: successor_body<0>(p, lds); break;
    case 1: successor_body<1>(p, lds); break;
    case 2: successor_body<2>(p, lds); break;
    default: successor_body<3>(p, lds); break;
    }
}

// pmx_bot_query: what bot `code` computes for agent I on the current state and what it would play now; nothing is written back.
// It calls the very device functions the tick calls (bot_decide, random_legal).
template <int I, bool SIGHT>
__device__ __forceinline__ void bot_query_body(const PmxTickParams &p, uint32_t *lds, int code, double *values, int8_t *action,
                                               uint8_t *flags)
{
    Ctx c = make_ctx(p, lds);
    const int env = blockIdx.x * PMX_RULE_BLOCK + threadIdx.x;
    if (env >= p.N) return;
    Env e;
    load_env(e, c, p.state, p.N, env);
    const int legal = legal_mask(c.wl, c.wls, (int)(e.xy[I] & 0xFF), (int)(e.xy[I] >> 8));
    double v[5] = { 0.0, 0.0, 0.0, 0.0, 0.0 };
    int r;
    if (code == -2 || !c.dist) r = random_legal(legal, c.rng_key, e.ticks, I);      // (the host refuses other codes without bots)
    else r = bot_decide<I, SIGHT>(e, c, code, v, p.bot_sight);
    if (values) {
#pragma unroll
        for (int a = 0; a < 5; ++a) values[5 * (size_t)env + a] = ((legal >> a) & 1) ? v[a] : __longlong_as_double(0x7FF8000000000000LL);
    }
    if (action) action[env] = (int8_t)(r & 0xFF);
    if (flags) flags[env] = (uint8_t)(r >> 8);
}

extern "C" __global__ __launch_bounds__(PMX_RULE_BLOCK) void pmx_bot_query_kernel(PmxTickParams p, int agent, int code, double *values,
                                                                                  int8_t *action, uint8_t *flags)
{
    extern __shared__ uint32_t lds[];
    switch (agent) {   // wave-uniform
    case 0: bot_query_body<0, false>(p, lds, code, values, action, flags); break;
    case 1: bot_query_body<1, false>(p, lds, code, values, action, flags); break;
    case 2: bot_query_body<2, false>(p, lds, code, values, action, flags); break;
    default: bot_query_body<3, false>(p, lds, code, values, action, flags); break;
    }
}
// its twin for handles with a bot sight: the flags also carry PMX_BOT_SEEN_LO / _HI
extern "C" __global__ __launch_bounds__(PMX_RULE_BLOCK) void pmx_bot_query_sight_kernel(PmxTickParams p, int agent, int code, double *values,
                                                                                        int8_t *action, uint8_t *flags)
{
    extern __shared__ uint32_t lds[];
    switch (agent) {   // wave-uniform
    case 0: bot_query_body<0, true>(p, lds, code, values, action, flags); break;
    case 1: bot_query_body<1, true>(p, lds, code, values, action, flags); break;
    case 2: bot_query_body<2, true>(p, lds, code, values, action, flags); break;
    default: bot_query_body<3, true>(p, lds, code, values, action, flags); break;
    }
}

template <bool BOTS>
__global__ __launch_bounds__(PMX_RULE_BLOCK) void pmx_rule_agent_kernel(PmxTickParams p, int agent)
{
    extern __shared__ uint32_t lds[];
    switch (agent) {   // wave-uniform
    case 0: rule_agent_body<0, BOTS ? 1 : 0>(p, lds); break;
    case 1: rule_agent_body<1, BOTS ? 1 : 0>(p, lds); break;
    case 2: rule_agent_body<2, BOTS ? 1 : 0>(p, lds); break;
    default: rule_agent_body<3, BOTS ? 1 : 0>(p, lds); break;
    }
}
__global__ __launch_bounds__(PMX_RULE_BLOCK) void pmx_rule_agent_sight_kernel(PmxTickParams p, int agent)
{
    extern __shared__ uint32_t lds[];
    switch (agent) {   // wave-uniform
    case 0: rule_agent_body<0, 2>(p, lds); break;
    case 1: rule_agent_body<1, 2>(p, lds); break;
    case 2: rule_agent_body<2, 2>(p, lds); break;
    default: rule_agent_body<3, 2>(p, lds); break;
    }
}

// gymPacMan.reset (gymPacMan.py:92-141) for the masked envs; legal masks for all envs if requested
extern "C" __global__ __launch_bounds__(PMX_RULE_BLOCK) void pmx_reset_kernel(PmxTickParams p)
{
    extern __shared__ uint32_t lds[];
    Ctx c = make_ctx(p, lds);
    const int env = blockIdx.x * PMX_RULE_BLOCK + threadIdx.x;
    if (env >= p.N) return;
    Env e;
    if (!p.no_reset && (!p.reset_mask || p.reset_mask[env])) {
        e.ticks = p.state[(size_t)PMX_W_TICKS(c.H) * p.N + env];
        if (p.layout_idx_rw) switch_layout(c, p, env, redraw_layout(c.rng_key, e.ticks, p.n_layouts));
        init_env(e, c);
        store_env(e, c, p.state, p.N, env);
        for (int k = 0; k < 7; ++k) p.state[(size_t)(PMX_W_ACC(c.H) + k) * p.N + env] = 0;
    } else if (p.legal) {
        load_env(e, c, p.state, p.N, env);
    }
    if (p.legal) {
        uint32_t m = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) m |= (uint32_t)legal_mask(c.wl, c.wls, (int)(e.xy[i] & 0xFF), (int)(e.xy[i] >> 8)) << (8 * i);
        reinterpret_cast<uint32_t *>(p.legal)[env] = m;
    }
}

template <int DT> struct ObsVec;
template <> struct ObsVec<0> { static constexpr int VEC = 4; };    // float32
template <> struct ObsVec<1> { static constexpr int VEC = 8; };    // bfloat16
template <> struct ObsVec<2> { static constexpr int VEC = 16; };   // uint8

// VEC stream bits (bit j = element j of the 16-byte vector) -> the 16 bytes.  Set elements are 1 in the output type.
template <int DT>
__device__ __forceinline__ uint4 pack_obs(uint32_t bits)
{
    uint32_t w[4];
    if (DT == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = (uint32_t)__builtin_amdgcn_sbfe((int)bits, j, 1) & 0x3F800000u;
    } else if (DT == 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            w[k] = ((uint32_t)__builtin_amdgcn_sbfe((int)bits, 2 * k, 1) & 0x3F80u) |
                   ((uint32_t)__builtin_amdgcn_sbfe((int)bits, 2 * k + 1, 1) & 0x3F800000u);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = (((bits >> (4 * k)) & 0xFu) * 0x00204081u) & 0x01010101u;   // bit j -> byte j
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// ---------------------------------------------------------------------------------------------------------------
// Wall writer of the rule launch (pmx_rule_kernel, blocks behind the rule blocks).  Plane 0 of every (env, emitted agent)
// block is the layout's wall_stream expanded to float32 (the split is used for float32 planes only, see pmx_step).  One wave
// per block walks the (env, agent) blocks grid-stride and stores the block's first wall_split_vec(block, first_vec) vectors
// (pmx_device.h): of the first_vec = H*W*4 / 16 vectors that lie WHOLLY inside plane 0, those in front of the last 128-byte
// line boundary of the block's address.  The wall-only vectors behind that boundary, the
// vector that plane 0 shares with plane 1, and everything behind it, belong to pmx_expand_kernel (PmxExpandParams::first_vec).
// With one layout the vectors are computed once per wave and only stored again; with per-env layouts they are recomputed
// from the env's layout record.  A lane holds vector lane + 64 j; the largest board (32 x 32) needs j < 4.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void write_walls(const PmxTickParams &p)
{
    constexpr int VEC = ObsVec<0>::VEC;
    constexpr int MAXJ = 32 * 32 / VEC / 64;
    const int lane = threadIdx.x;
    const int HW = p.lay_H * p.lay_W;
    const int first_vec = HW / VEC;
    const size_t n_vec = (size_t)(8 * HW / VEC);
    const long total = (long)p.N * p.n_emit;
    const long stride = (long)gridDim.x - p.rule_blocks;
    uint4 v[MAXJ];
    auto pack = [&](const PmxLayoutDev *L) {
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) {
            const uint32_t e0 = (uint32_t)(lane + 64 * j) * VEC;       // < 32 * 32: always inside wall_stream
            v[j] = pack_obs<0>(L->wall_stream[e0 >> 5] >> (e0 & 31));
        }
    };
    if (!p.layout_idx) pack(p.lay);
    for (long q = (long)blockIdx.x - p.rule_blocks; q < total; q += stride) {
        if (p.layout_idx) pack(p.lay + p.layout_idx[q / p.n_emit]);
        uint4 *out = reinterpret_cast<uint4 *>(p.obs) + (size_t)q * n_vec;
        const int split = wall_split_vec(out, first_vec);
#pragma unroll
        for (int j = 0; j < MAXJ; ++j)
            if (lane + 64 * j < split) {   // streaming stores (one dwordx4 nt): see the measurements at pmx_launch_rule
                uint4 *o = &out[lane + 64 * j];
                __builtin_nontemporal_store(v[j].x, &o->x); __builtin_nontemporal_store(v[j].y, &o->y);
                __builtin_nontemporal_store(v[j].z, &o->z); __builtin_nontemporal_store(v[j].w, &o->w);
            }
    }
}

// the one element of plane 1 that is set holds 1 + numCarrying (gymPacMan.py:205): patch element d of the vector
template <int DT>
__device__ __forceinline__ void patch_self(uint4 &v, int d, uint32_t carry)
{
    // uint8: selects on the four members, never an index into the vector: the compiler turns the unrolled loop of
    // `if (k == d >> 2) w[k] += ..` into a dynamically indexed access to a copy of the vector in SCRATCH memory, and every
    // scratch reload waits for vmcnt(0), i.e. for all the plane stores in flight (the uint8 kernels did exactly that; the
    // float32 / bfloat16 forms below compile to compares and selects and stay as they are)
    if (DT == 0) {
        uint32_t *w = reinterpret_cast<uint32_t *>(&v);
        const uint32_t val = __float_as_uint((float)(1 + carry));
#pragma unroll
        for (int j = 0; j < 4; ++j) if (d == j) w[j] = val;
    } else if (DT == 1) {
        uint32_t *w = reinterpret_cast<uint32_t *>(&v);
        const uint32_t val = __float_as_uint((float)(1 + carry)) >> 16;   // exact in bfloat16 for 1 + carry <= 256
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (d == 2 * k) w[k] = (w[k] & 0xFFFF0000u) | val;
            if (d == 2 * k + 1) w[k] = (w[k] & 0x0000FFFFu) | (val << 16);
        }
    } else {
        const uint32_t add = carry << (8 * (d & 3));
        const int k = d >> 2;
        v.x += k == 0 ? add : 0u; v.y += k == 1 ? add : 0u; v.z += k == 2 ? add : 0u; v.w += k == 3 ? add : 0u;
    }
}

// OR the W-bit row `v` into the packed bit stream at bit offset `off`
__device__ __forceinline__ void stream_or_row(uint32_t *T, uint32_t off, uint32_t v, int W)
{
    if (v == 0) return;
    const uint32_t word = off >> 5, sh = off & 31;
    atomicOr(&T[word], v << sh);
    if (sh + W > 32) atomicOr(&T[word + 1], v >> (32 - sh));
}

// ---------------------------------------------------------------------------------------------------------------
// Observation expansion (gymPacMan.py:195-229).  One wavefront per (env, emitted agent), wavefronts independent.
//   1. the wave assembles the PACKED bit stream of the [8][H][W] block in LDS (bit e = element e != 0): the wall
//      plane is a per-layout constant copied from the layout record, the food planes are OR-ed in row by row
//      (H lanes), self / ally / enemies / capsules are single bits (8 lanes);
//   2. every lane then reads ONE aligned stream word per 16 output bytes (a 4/8/16-bit field never straddles a
//      32-bit word), turns its bits into the 16 bytes through a block-shared look-up table and issues one dwordx4
//      store: the wave writes 1 KiB of consecutive addresses per instruction.  LDS operations of one wavefront
//      execute in order, so the waves need no barrier after the one that publishes the look-up table.
// ---------------------------------------------------------------------------------------------------------------
// The 16 output bytes of a lane come from a block-shared lookup table indexed by its stream bits (float32: 16 entries
// of 16 bytes, every entry in its own four LDS banks, so any mix of indices is conflict free; bfloat16: 256 entries; uint8: two
// 8-bit look-ups of 8 bytes) instead of being computed: with the observation buffer partly resident in the Infinity Cache the
// float32 kernel had become instruction bound (~1.8 T elements/s whatever the footprint), and the expansion arithmetic was most
// of its ~35 instructions per 16 bytes.
// BEHIND (float32, ordinary stores): the store loop starts at wall_split_vec(block, H*W*4/16), behind the wall vectors the rule
// launch stored, i.e. on a 128-byte line of the block's address; the wall-only vectors from there to the end of plane 0 come
// out of the stream table like every other vector.  (PmxExpandParams::first_vec > 0 only selects this instantiation.)  A
// template flag and not a test of first_vec, so that the full-plane instantiations are the code they were without the split.
// SIGHT (pmx_set_obs_sight; include/pmx.h, "Sight rule on the four-agent planes"): the contest's sight rule on the block of agent
// `agent`.  Lanes 0-3 hold the four agent words already; lane l takes P[agent] and P[agent ^ 2] from them by two wave shuffles and,
// when its agent is an enemy further than `sight` from both, skips its atomicOr into the stream table.  No load, no LDS and no
// store is added or changed.  Everything is under `if constexpr (SIGHT)`, and the body is shared by two kernels, so that
// pmx_expand_kernel's instantiations stay the code they were (profiles/obs_sight/resource_usage.txt).
template <int DT, bool NT, bool BEHIND, bool SIGHT>
__device__ __forceinline__ void expand_block(const PmxExpandParams &p, [[maybe_unused]] int sight)
{
    constexpr int VEC = ObsVec<DT>::VEC;
    __shared__ uint32_t tab[4][8 * 32 * 32 / 32 + 8];
    __shared__ __align__(16) uint32_t lut[DT == 0 ? 16 * 4 : (DT == 1 ? 256 * 4 : 256 * 2)];
    {
        const uint32_t i = threadIdx.x;
        if (DT == 0) {
            if (i < 16) *reinterpret_cast<uint4 *>(&lut[4 * i]) = pack_obs<0>(i);
        } else if (DT == 1) {
            *reinterpret_cast<uint4 *>(&lut[4 * i]) = pack_obs<1>(i);
        } else {
            lut[2 * i] = ((i & 15u) * 0x00204081u) & 0x01010101u;
            lut[2 * i + 1] = ((i >> 4) * 0x00204081u) & 0x01010101u;
        }
        __syncthreads();
    }
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int W = p.lay_W, H = p.lay_H;
    const int HW = H * W;
    const long total = (long)p.N * p.n_emit;
    long blk = p.reverse ? (long)gridDim.x - 1 - (long)blockIdx.x : (long)blockIdx.x;
    if (p.n_emit == 4 && (p.N & 127) == 0) {
        // XCD-aware order: blocks b, b+8, b+16, .. share an XCD and its L2.  Give each XCD 16 consecutive envs, i.e. the
        // envs whose SoA snapshot words share 64-byte lines, so that a line is fetched into one L2 instead of eight
        // (PMC: FETCH_SIZE per launch drops accordingly; wall time is unchanged, the kernel is store-bound).
        const long g = blk >> 7, r = blk & 127;
        blk = (g << 7) + ((r & 7) << 4) + (r >> 3);
    }
    const long q = blk * 4 + wave;
    if (q >= total) return;
    const long env = q / p.n_emit;
    const int slot = (int)(q - env * p.n_emit);
    const int agent = p.single_agent >= 0 ? p.single_agent : p.emit[slot];
    const uint32_t *S = p.snap[agent] + env;
    const size_t N = (size_t)p.N;
    uint32_t *T = tab[wave];
    const PmxLayoutDev *L = p.lay + (p.layout_idx ? p.layout_idx[env] : 0);

    // issue the snapshot loads first, their latency hides behind the table initialisation
    const uint32_t food = lane < H ? S[(size_t)lane * N] : 0u;
    uint32_t pt = 0;
    if (lane < 4) pt = S[(size_t)PMX_W_AGENT_A(H, lane) * N];
    else if (lane < 8) pt = S[(size_t)PMX_W_CAPS(H, (lane - 4) >> 1) * N];
    const uint32_t a_self = S[(size_t)PMX_W_AGENT_A(H, agent) * N];
    const uint32_t b_self = S[(size_t)PMX_W_AGENT_B(H, agent) * N];

    const int n_words = (8 * HW + 31) >> 5;
    const int wall_words = (HW + 31) >> 5;
    for (int k = lane; k < n_words + 1; k += 64) T[k] = k < wall_words ? L->wall_stream[k] : 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < H) {
        stream_or_row(T, (uint32_t)((6 * H + lane) * W), food & L->hi_mask, W);    // blue food: x >= int(W/2) (capture.py:336)
        stream_or_row(T, (uint32_t)((7 * H + lane) * W), food & L->lo_mask, W);    // red food
    }
    [[maybe_unused]] uint32_t ps = 0, pm = 0;                                        // SIGHT: word A of the agent and of its mate
    if constexpr (SIGHT) {                                                          // (every lane of the wave runs the shuffles)
        ps = (uint32_t)__shfl((int)pt, agent);
        pm = (uint32_t)__shfl((int)pt, agent ^ 2);
    }
    if (lane < 4) {
        const int x = pt & 0xFF, y = (pt >> 8) & 0xFF;
        const int plane = lane == agent ? 1 : (((lane ^ agent) == 2) ? 4 : 5);      // gymPacMan.py:205-215
        const uint32_t off = (uint32_t)((plane * H + y) * W + x);
        bool shown = true;
        if constexpr (SIGHT) {                                                          // capture.py:285-291
            const int da = abs(x - (int)(ps & 0xFF)) + abs(y - (int)((ps >> 8) & 0xFF));
            const int dm = abs(x - (int)(pm & 0xFF)) + abs(y - (int)((pm >> 8) & 0xFF));
            shown = plane != 5 || (da < dm ? da : dm) <= sight;
        }
        if (shown) atomicOr(&T[off >> 5], 1u << (off & 31));
    } else if (lane < 8) {
        const uint32_t cxy = (pt >> (16 * ((lane - 4) & 1))) & 0xFFFFu;
        if (cxy != 0xFFFFu) {
            const int x = cxy & 0xFF, y = cxy >> 8;
            const int plane = (2 * x > W) ? 2 : 3;                                  // halfList: blue x > W/2, red x <= W/2
            const uint32_t off = (uint32_t)((plane * H + y) * W + x);
            atomicOr(&T[off >> 5], 1u << (off & 31));
        }
    }
    const uint32_t carry = (b_self >> 8) & 0xFFF;
    const int fself = (H + (int)((a_self >> 8) & 0xFF)) * W + (int)(a_self & 0xFF);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    const int n_vec = 8 * HW / VEC;
    uint4 *out = reinterpret_cast<uint4 *>(p.obs) + (size_t)q * n_vec;
    for (int k = (BEHIND ? wall_split_vec(out, HW * (int)sizeof(float) / 16) : 0) + lane; k < n_vec; k += 64) {
        const uint32_t e0 = (uint32_t)k * VEC;
        const uint32_t bits = T[e0 >> 5] >> (e0 & 31);
        uint4 v;
        if (DT == 0) v = *reinterpret_cast<const uint4 *>(&lut[(bits & 15u) * 4]);
        else if (DT == 1) v = *reinterpret_cast<const uint4 *>(&lut[(bits & 255u) * 4]);
        else {
            const uint2 lo = *reinterpret_cast<const uint2 *>(&lut[(bits & 255u) * 2]);
            const uint2 hi = *reinterpret_cast<const uint2 *>(&lut[((bits >> 8) & 255u) * 2]);
            v = make_uint4(lo.x, lo.y, hi.x, hi.y);
        }
        const uint32_t d = (uint32_t)(fself - (int)e0);
        if (d < (uint32_t)VEC) patch_self<DT>(v, (int)d, carry);
        if (NT) {   // streaming stores (merged into one dwordx4 nt): used when the planes exceed the Infinity Cache
            __builtin_nontemporal_store(v.x, &out[k].x); __builtin_nontemporal_store(v.y, &out[k].y);
            __builtin_nontemporal_store(v.z, &out[k].z); __builtin_nontemporal_store(v.w, &out[k].w);
        } else {
            out[k] = v;
        }
    }
}

template <int DT, bool NT, bool BEHIND = false>
__global__ __launch_bounds__(PMX_BLOCK) void pmx_expand_kernel(PmxExpandParams p)
{
    expand_block<DT, NT, BEHIND, false>(p, 0);
}

// the sight form (handles with pmx_set_obs_sight): always the full block, the wall split is not taken with it
template <int DT, bool NT>
__global__ __launch_bounds__(PMX_BLOCK) void pmx_expand_sight_kernel(PmxExpandParams p, int sight)
{
    expand_block<DT, NT, false, true>(p, sight);
}

// ---------------------------------------------------------------------------------------------------------------
// The whole tick in ONE launch (pmx_step with float32 planes, all four agents, one layout, no bots, H <= 20, N % 64 == 0 and at
// least one workgroup per CU: pmx_step's fused_min_envs).  Workgroup g owns envs 64 g .. 64 g + 63 from the state load to the last
// plane byte: no workgroup reads what another one wrote in this launch, and the only synchronisation is TWO __syncthreads().
//   phase A0 wave 0 loads the state of its 64 envs and runs sub-step 0 with pmx_rule_kernel's device functions and lane mapping;
//            where that kernel stores a snapshot to global memory, this one copies the H + 10 words into the LDS area
//            snap[4][..][64].  Waves 1-15 store the wall vectors of the workgroup's 256 (env, agent) blocks with streaming
//            stores, as write_walls does: those in front of the block's wall_split_vec, a 128-byte line of its address, so
//            that every store instruction of the expansion behind it covers 8 whole lines.  Barrier.
//   phase A1 wave 0 runs sub-steps 1-3 and tick_finish (slots 1, 2 and, with the H + 13 words of the final state, 3); waves 1-15
//            expand the 64 agent-0 blocks from slot 0, which is complete: HBM has plane bytes to store while the rule wave runs.
//            An env that finishes shows the fresh game to all four agents, so its agent-0 block is stale: wave 0 writes the fresh
//            game to slots 1 and 2 (NOT to slot 0, which the other waves are reading) and leaves the ballot of such envs in LDS.
//            Barrier.
//   phase B  wave 0 copies slot 1 over slot 0 for the envs of the ballot and writes slot 0 to p.snap, the other waves write slots
//            1-3 to p.snap / p.state with 16-byte stores (pmx_observe, pmx_emit_team_obs, pmx_step_agent and the next tick read
//            them there); every wave expands the agent-0 blocks of the ballot it stored in A1 again, from slot 1 (the same lane
//            stores to the same address twice, in program order); the 192 blocks of agents 1-3 are dealt to the 16 waves, and
//            each is expanded as pmx_expand_kernel<0, false, true> expands it, the snapshot words coming from LDS.
// What the two launches cost and this one does not: the end-of-kernel write-back and the second dispatch, and the snapshot
// round trip through memory in front of every expansion wave.  No global load is issued by waves 1-15, or by any wave in phase
// B: loads return in order behind the stores in front of them, and a wave that waited for one would wait for its plane stores.
// (That is also why the wall words of the stream tables come from an LDS copy of the layout's wall_stream.)
// LDS (dynamic): make_ctx's area | snap | look-up table (16 x 16 bytes) | wall_stream (32 words) | ballot (2 words + 2 of
// padding) | 16 stream tables of fused_tab_stride words.
// ---------------------------------------------------------------------------------------------------------------
#define PMX_FUSED_WAVES 16
__host__ __device__ inline int fused_rule_words(int H) { return 32 + (3 * H + 16) * PMX_RULE_BLOCK; }
__host__ __device__ inline int fused_snap_rows(int H) { return 3 * PMX_SNAP_WORDS(H) + H + 13; }
__host__ __device__ inline int fused_tab_stride(int H, int W) { return (((8 * H * W + 31) >> 5) + 1 + 3) & ~3; }

// the snapshot words of this lane's env -> column `slot` (= slot base + lane) of the LDS snapshot area; FULL: + score, steps, ticks
template <int HB, bool FULL>
__device__ __forceinline__ void snapshot_to_lds(const Env &e, const Ctx &c, uint32_t *slot)
{
    uint32_t rows[HB];
#pragma unroll
    for (int y = 0; y < HB; ++y) rows[y] = y < c.H ? c.fd[y * PMX_RULE_BLOCK] : 0u;
#pragma unroll
    for (int y = 0; y < HB; ++y)
        if (y < c.H) slot[y * PMX_RULE_BLOCK] = rows[y];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        slot[PMX_W_AGENT_A(c.H, i) * PMX_RULE_BLOCK] = pack_a(e, i);
        slot[PMX_W_AGENT_B(c.H, i) * PMX_RULE_BLOCK] = pack_b(e, i);
    }
    slot[PMX_W_CAPS(c.H, 0) * PMX_RULE_BLOCK] = e.capw[0];
    slot[PMX_W_CAPS(c.H, 1) * PMX_RULE_BLOCK] = e.capw[1];
    if (FULL) {
        slot[PMX_W_SCORE(c.H) * PMX_RULE_BLOCK] = (uint32_t)e.score;
        slot[PMX_W_STEPS(c.H) * PMX_RULE_BLOCK] = (uint32_t)e.steps;
        slot[PMX_W_TICKS(c.H) * PMX_RULE_BLOCK] = e.ticks;
    }
}

// One wave expands the planes behind the wall vectors of one (env, agent) block: S = the env's column of the snapshot slot,
// T = the wave's stream table, out = the block.  Ordinary stores from wall_split_vec(out, first_vec) on: whole 128-byte lines.
__device__ __forceinline__ void fused_expand_block(const PmxTickParams &p, const uint32_t *S, int agent, uint32_t *T, const uint32_t *lut,
                                                   uint32_t wallw, uint4 *out, int lane)
{
    constexpr int VEC = ObsVec<0>::VEC;
    const int H = p.lay_H, W = p.lay_W, HW = H * W;
    const int first_vec = HW / VEC, n_vec = 8 * HW / VEC, n_words = (8 * HW + 31) >> 5;
    const uint32_t food = lane < H ? S[lane * PMX_RULE_BLOCK] : 0u;
    uint32_t pt = 0;
    if (lane < 4) pt = S[PMX_W_AGENT_A(H, lane) * PMX_RULE_BLOCK];
    else if (lane < 8) pt = S[PMX_W_CAPS(H, (lane - 4) >> 1) * PMX_RULE_BLOCK];
    const uint32_t a_self = S[PMX_W_AGENT_A(H, agent) * PMX_RULE_BLOCK];
    const uint32_t b_self = S[PMX_W_AGENT_B(H, agent) * PMX_RULE_BLOCK];
    for (int k = lane; k < n_words + 1; k += 64) T[k] = k < 32 ? wallw : 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < H) {
        stream_or_row(T, (uint32_t)((6 * H + lane) * W), food & p.hi_mask, W);    // blue food: x >= int(W/2) (capture.py:336)
        stream_or_row(T, (uint32_t)((7 * H + lane) * W), food & p.lo_mask, W);    // red food
    }
    if (lane < 4) {
        const int x = pt & 0xFF, y = (pt >> 8) & 0xFF;
        const int plane = lane == agent ? 1 : (((lane ^ agent) == 2) ? 4 : 5);      // gymPacMan.py:205-215
        const uint32_t off = (uint32_t)((plane * H + y) * W + x);
        atomicOr(&T[off >> 5], 1u << (off & 31));
    } else if (lane < 8) {
        const uint32_t cxy = (pt >> (16 * ((lane - 4) & 1))) & 0xFFFFu;
        if (cxy != 0xFFFFu) {
            const int x = cxy & 0xFF, y = cxy >> 8;
            const int plane = (2 * x > W) ? 2 : 3;                                  // halfList: blue x > W/2, red x <= W/2
            const uint32_t off = (uint32_t)((plane * H + y) * W + x);
            atomicOr(&T[off >> 5], 1u << (off & 31));
        }
    }
    const uint32_t carry = (b_self >> 8) & 0xFFF;
    const int fself = (H + (int)((a_self >> 8) & 0xFF)) * W + (int)(a_self & 0xFF);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    for (int k = wall_split_vec(out, first_vec) + lane; k < n_vec; k += 64) {
        const uint32_t e0 = (uint32_t)k * VEC;
        const uint32_t bits = T[e0 >> 5] >> (e0 & 31);
        uint4 v = *reinterpret_cast<const uint4 *>(&lut[(bits & 15u) * 4]);
        const uint32_t d = (uint32_t)(fself - (int)e0);
        if (d < (uint32_t)VEC) patch_self<0>(v, (int)d, carry);
        out[k] = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // the table is rewritten for the next block
    __builtin_amdgcn_wave_barrier();
}

template <int HB>
__global__ __launch_bounds__(PMX_FUSED_WAVES * 64) void pmx_tick_fused_kernel(PmxTickParams p, int reverse)
{
    constexpr int VEC = ObsVec<0>::VEC, NB = 4 * PMX_RULE_BLOCK;   // (env, agent) blocks of a workgroup
    extern __shared__ uint32_t lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int H = p.lay_H, W = p.lay_W, HW = H * W;
    // reverse (the alternating sweep, pmx_launch_expand): the workgroups take the groups, and the waves their blocks, backwards
    const int group = reverse ? (int)gridDim.x - 1 - (int)blockIdx.x : (int)blockIdx.x;
    uint32_t *snapL = lds + fused_rule_words(H);
    uint32_t *lut = snapL + fused_snap_rows(H) * PMX_RULE_BLOCK;
    uint32_t *wstream = lut + 64;                                    // the layout's wall_stream: plane 0 of every stream table
    uint32_t *freshL = wstream + 32;                                 // the ballot of the envs that finished in this tick
    uint32_t *T = freshL + 4 + wave * fused_tab_stride(H, W);
    const int slot_words = PMX_SNAP_WORDS(H) * PMX_RULE_BLOCK;
    const int first_vec = HW / VEC, n_vec = 8 * HW / VEC;
    uint4 *obs = reinterpret_cast<uint4 *>(p.obs) + (size_t)group * NB * n_vec;
    const int env = group * PMX_RULE_BLOCK + lane;

    // what the rule wave keeps across the first barrier (wave 0 only; both branches on `wave` are wave-uniform)
    Env e;
    Acc a = { 0.0, 0.0, 0, 0, 0, 0, 0 };
    Ctx c;
    uint32_t av = 0;
    uint32_t *col = snapL + lane;

    // ---- phase A0 ----
    if (wave == 0) {
        RawEnv raw;
        uint32_t rows[HB];
        load_env_issue<HB>(raw, rows, p.state, p.N, env, H);
        av = reinterpret_cast<const uint32_t *>(p.actions)[env];   // 4 int8 actions
        c = make_ctx_fill(p, lds, env, lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // the wall rows: only this wave reads them
        __builtin_amdgcn_wave_barrier();
        load_env_commit<HB>(e, c, raw, rows);
        count_food<HB>(a, c, rows);
        tick_substep<0, false>(e, a, c, (int)(int8_t)(av & 0xFF));
        snapshot_to_lds<HB, false>(e, c, col);
    } else {
        constexpr int MAXJ = 32 * 32 / VEC / 64;
        if (wave == 1 && lane < 16) *reinterpret_cast<uint4 *>(&lut[4 * lane]) = pack_obs<0>(lane);
        if (wave == 1 && lane < 32) wstream[lane] = p.lay->wall_stream[lane];
        uint4 v[MAXJ];
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) {
            const uint32_t e0 = (uint32_t)(lane + 64 * j) * VEC;       // < 32 * 32: always inside wall_stream
            v[j] = pack_obs<0>(p.lay->wall_stream[e0 >> 5] >> (e0 & 31));
        }
        for (int b = wave - 1; b < NB; b += PMX_FUSED_WAVES - 1) {
            uint4 *out = obs + (size_t)(reverse ? NB - 1 - b : b) * n_vec;
            const int split = wall_split_vec(out, first_vec);
#pragma unroll
            for (int j = 0; j < MAXJ; ++j)
                if (lane + 64 * j < split) {   // streaming stores, as in write_walls
                    uint4 *o = &out[lane + 64 * j];
                    __builtin_nontemporal_store(v[j].x, &o->x); __builtin_nontemporal_store(v[j].y, &o->y);
                    __builtin_nontemporal_store(v[j].z, &o->z); __builtin_nontemporal_store(v[j].w, &o->w);
                }
        }
    }
    __syncthreads();

    // ---- phase A1: slot 0, the look-up table and wstream are complete ----
    const uint32_t wallw = lane < 32 ? wstream[lane] : 0u;           // (zero behind the H*W wall bits)
    if (wave == 0) {
        tick_substep<1, false>(e, a, c, (int)(int8_t)((av >> 8) & 0xFF));
        snapshot_to_lds<HB, false>(e, c, col + slot_words);
        tick_substep<2, false>(e, a, c, (int)(int8_t)((av >> 16) & 0xFF));
        snapshot_to_lds<HB, false>(e, c, col + 2 * slot_words);
        tick_substep<3, false>(e, a, c, (int)(int8_t)((av >> 24) & 0xFF));
        const bool fresh = tick_finish<HB, false>(e, a, c, p, env, true);
        snapshot_to_lds<HB, true>(e, c, col + 3 * slot_words);
        if (fresh) {   // the observations of a finished env are those of the fresh game for all four agents; slot 0 follows in
                       // phase B, when no wave reads it any more
            snapshot_to_lds<HB, false>(e, c, col + slot_words);
            snapshot_to_lds<HB, false>(e, c, col + 2 * slot_words);
        }
        const unsigned long long fb = __ballot(fresh);
        if (lane == 0) { freshL[0] = (uint32_t)fb; freshL[1] = (uint32_t)(fb >> 32); }
    } else {
        for (int j = wave - 1; j < PMX_RULE_BLOCK; j += PMX_FUSED_WAVES - 1) {
            const int el = reverse ? PMX_RULE_BLOCK - 1 - j : j;
            fused_expand_block(p, snapL + el, 0, T, lut, wallw, obs + (size_t)(4 * el) * n_vec, lane);
        }
    }
    __syncthreads();

    // ---- phase B ----
    {   // the four slots -> p.snap[0..2] and p.state: rows of 64 envs = 16 vectors of 16 bytes, [3][H + 10][N] is one row range.
        // Slot 0 is wave 0's: it first gives the envs that finished the fresh game there (slot 1 holds it), in program order.
        const int n_rows = fused_snap_rows(H), rows0 = PMX_SNAP_WORDS(H), snap_rows = 3 * rows0;
        int i, i_end, i_step;
        if (wave == 0) {
            if ((lane < 32 ? freshL[0] >> lane : freshL[1] >> (lane - 32)) & 1u)
                for (int r = 0; r < rows0; ++r) col[r * PMX_RULE_BLOCK] = col[slot_words + r * PMX_RULE_BLOCK];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            i = lane; i_end = rows0 * 16; i_step = 64;
        } else {
            i = rows0 * 16 + (int)threadIdx.x - 64; i_end = n_rows * 16; i_step = (PMX_FUSED_WAVES - 1) * 64;
        }
        for (; i < i_end; i += i_step) {
            const int row = i >> 4, q4 = 4 * (i & 15);
            const uint4 w = *reinterpret_cast<const uint4 *>(snapL + row * PMX_RULE_BLOCK + q4);
            uint32_t *dst = row < snap_rows ? p.snap + (size_t)row * p.N : p.state + (size_t)(row - snap_rows) * p.N;
            *reinterpret_cast<uint4 *>(dst + (size_t)group * PMX_RULE_BLOCK + q4) = w;
        }
    }

    // the agent-0 blocks of the envs that finished, again and by the wave that stored them in A1: from slot 1, the fresh game
    const uint32_t fresh_lo = __builtin_amdgcn_readfirstlane(freshL[0]), fresh_hi = __builtin_amdgcn_readfirstlane(freshL[1]);
    if (wave != 0 && (fresh_lo | fresh_hi) != 0u) {
        for (int j = wave - 1; j < PMX_RULE_BLOCK; j += PMX_FUSED_WAVES - 1) {
            const int el = reverse ? PMX_RULE_BLOCK - 1 - j : j;
            if (((el < 32 ? fresh_lo >> el : fresh_hi >> (el - 32)) & 1u) == 0u) continue;
            fused_expand_block(p, snapL + slot_words + el, 0, T, lut, wallw, obs + (size_t)(4 * el) * n_vec, lane);
        }
    }

    // agents 1-3: 192 blocks over 16 waves, an env's three blocks on neighbouring waves (their shared 128-byte lines are stored
    // close together in time)
    constexpr int NB3 = 3 * PMX_RULE_BLOCK;
    for (int it = 0; it < NB3 / PMX_FUSED_WAVES; ++it) {
        const int b = it * PMX_FUSED_WAVES + wave;
        const int m = reverse ? NB3 - 1 - b : b;
        const int el = m / 3, agent = 1 + m - 3 * el;
        fused_expand_block(p, snapL + agent * slot_words + el, agent, T, lut, wallw, obs + (size_t)(4 * el + agent) * n_vec, lane);   // agent 3: the final state
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The same expansion with ONE wavefront per ENV for uint8 planes: at 1 byte per element an (env, agent) block is 1.2 KB, i.e.
// one or two store instructions per lane behind a fixed ~2 us of snapshot-load latency and table set-up -- pmx_expand_kernel is
// issue / latency bound there (0.39 of the HBM peak).  Here a wave issues the snapshot loads of all four agents together, builds
// the four bit streams side by side in LDS and then streams the env's whole [4][8][H][W] block (4.9 KB for smallCapture,
// contiguous: whole 128-byte lines except at the two ends, where pmx_expand_kernel's 1 232-byte agent blocks split a line each).
// ---------------------------------------------------------------------------------------------------------------
// One env per wave.  Measured and not kept: two envs per wave, the second env's snapshot words loaded while the first env's
// planes are streamed (a wave spent ~7 k of its ~14 k shader-clock ticks on the snapshot loads, which queue behind the other
// waves' plane stores), ran 20.4 us against 18.5 us -- as did 16 envs per block with cooperative, fully coalesced snapshot
// loads (24.9 us): with half the waves the chip has fewer store streams in flight, and that costs more than the hidden latency.
struct SnapWords { uint32_t food[4], pt[4], a_self[4], b_self[4]; };
__device__ __forceinline__ void load_snap_words(SnapWords &s, const PmxExpandParams &p, long env, int lane, int H)
{
    const size_t N = (size_t)p.N;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const uint32_t *S = p.snap[a] + env;
        s.food[a] = lane < H ? S[(size_t)lane * N] : 0u;
        s.pt[a] = 0;
        if (lane < 4) s.pt[a] = S[(size_t)PMX_W_AGENT_A(H, lane) * N];
        else if (lane < 8) s.pt[a] = S[(size_t)PMX_W_CAPS(H, (lane - 4) >> 1) * N];
        s.a_self[a] = S[(size_t)PMX_W_AGENT_A(H, a) * N];
        s.b_self[a] = S[(size_t)PMX_W_AGENT_B(H, a) * N];
    }
}

template <bool NT>
__global__ __launch_bounds__(PMX_BLOCK) void pmx_expand4_kernel(PmxExpandParams p)
{
    constexpr int DT = 2, VEC = ObsVec<DT>::VEC;
    constexpr int TW = 8 * 32 * 32 / 32 + 8;
    __shared__ uint32_t tab[4][4][TW];                        // [wave][agent][stream words]
    __shared__ __align__(16) uint32_t lut[256 * 2];           // 8 stream bits -> 8 bytes
    {
        const uint32_t i = threadIdx.x;
        lut[2 * i] = ((i & 15u) * 0x00204081u) & 0x01010101u;
        lut[2 * i + 1] = ((i >> 4) * 0x00204081u) & 0x01010101u;
        __syncthreads();
    }
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int W = p.lay_W, H = p.lay_H, HW = H * W;
    long blk = p.reverse ? (long)gridDim.x - 1 - (long)blockIdx.x : (long)blockIdx.x;
    if ((p.N & 127) == 0) {
        // XCD-aware order (blocks b, b + 8, .. share an XCD): the 16 envs whose SoA snapshot words share a 64-byte line are
        // 4 consecutive blocks; send them to one XCD
        const long r = blk & 31;
        blk = (blk & ~31L) + (r & 7) * 4 + (r >> 3);
    }
    const long env = blk * 4 + wave;
    if (env >= p.N) return;
    const int n_words = (8 * HW + 31) >> 5;
    const int wall_words = (HW + 31) >> 5;
    const int n_vec = 8 * HW / VEC;
    SnapWords cur;
    load_snap_words(cur, p, env, lane, H);                    // all four agents' snapshot words in flight together
    const PmxLayoutDev *L = p.lay + (p.layout_idx ? p.layout_idx[env] : 0);
#pragma unroll
    for (int a = 0; a < 4; ++a)
        for (int k = lane; k < n_words + 1; k += 64) tab[wave][a][k] = k < wall_words ? L->wall_stream[k] : 0u;
    const uint32_t hi_mask = L->hi_mask, lo_mask = L->lo_mask;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    int fself[4];
    uint32_t carry[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        uint32_t *T = tab[wave][a];
        if (lane < H) {
            stream_or_row(T, (uint32_t)((6 * H + lane) * W), cur.food[a] & hi_mask, W);
            stream_or_row(T, (uint32_t)((7 * H + lane) * W), cur.food[a] & lo_mask, W);
        }
        if (lane < 4) {
            const int x = cur.pt[a] & 0xFF, y = (cur.pt[a] >> 8) & 0xFF;
            const int plane = lane == a ? 1 : (((lane ^ a) == 2) ? 4 : 5);
            const uint32_t off = (uint32_t)((plane * H + y) * W + x);
            atomicOr(&T[off >> 5], 1u << (off & 31));
        } else if (lane < 8) {
            const uint32_t cxy = (cur.pt[a] >> (16 * ((lane - 4) & 1))) & 0xFFFFu;
            if (cxy != 0xFFFFu) {
                const int x = cxy & 0xFF, y = cxy >> 8;
                const int plane = (2 * x > W) ? 2 : 3;
                const uint32_t off = (uint32_t)((plane * H + y) * W + x);
                atomicOr(&T[off >> 5], 1u << (off & 31));
            }
        }
        carry[a] = (cur.b_self[a] >> 8) & 0xFFF;
        fself[a] = (H + (int)((cur.a_self[a] >> 8) & 0xFF)) * W + (int)(cur.a_self[a] & 0xFF);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    uint4 *out = reinterpret_cast<uint4 *>(p.obs) + (size_t)env * 4 * n_vec;
    // U iterations of the store loop at a time: all their stream words are read first, then all look-up-table entries,
    // then the stores are issued -- one LDS round trip per group instead of two per 16 bytes (a wave spent 1.2 k ticks per
    // store instruction on these dependent reads)
    constexpr int U = 5;
    for (int base = 0; base < 4 * n_vec; base += 64 * U) {
        uint32_t bits[U];
        int ag[U];
        uint32_t e0s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kk = base + 64 * u + lane;
            const int a = (kk >= n_vec) + (kk >= 2 * n_vec) + (kk >= 3 * n_vec);
            const int a_c = kk < 4 * n_vec ? a : 0;
            const int k = kk < 4 * n_vec ? kk - a * n_vec : 0;
            ag[u] = a_c;
            e0s[u] = (uint32_t)k * VEC;
            bits[u] = tab[wave][a_c][e0s[u] >> 5] >> (e0s[u] & 31);
        }
        uint4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint2 lo = *reinterpret_cast<const uint2 *>(&lut[(bits[u] & 255u) * 2]);
            const uint2 hi = *reinterpret_cast<const uint2 *>(&lut[((bits[u] >> 8) & 255u) * 2]);
            v[u] = make_uint4(lo.x, lo.y, hi.x, hi.y);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kk = base + 64 * u + lane;
            const int a = ag[u];
            const int fs = a == 0 ? fself[0] : (a == 1 ? fself[1] : (a == 2 ? fself[2] : fself[3]));
            const uint32_t cr = a == 0 ? carry[0] : (a == 1 ? carry[1] : (a == 2 ? carry[2] : carry[3]));
            const uint32_t d = (uint32_t)(fs - (int)e0s[u]);
            if (d < (uint32_t)VEC) patch_self<DT>(v[u], (int)d, cr);
            if (kk < 4 * n_vec) {
                if (NT) {
                    __builtin_nontemporal_store(v[u].x, &out[kk].x); __builtin_nontemporal_store(v[u].y, &out[kk].y);
                    __builtin_nontemporal_store(v[u].z, &out[kk].z); __builtin_nontemporal_store(v[u].w, &out[kk].w);
                } else {
                    out[kk] = v[u];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Training-side emission: what the MAPPO rollout does with every tick's observations (pacman_mappo_resnet.py:462-469),
// straight from the snapshots: the two learners' planes -- canonicalised for a red team (canonicalize_obs :215-229: x
// flipped, capsule planes 2 <-> 3 and food planes 6 <-> 7 swapped) -- and merge_obs_for_critic (:267-274: the first
// learner's planes with plane 4 cleared and plane 1 = max of both learners' self planes).  Slots 0, 1 = the learners,
// slot 2 = the merged input; same packed-bit-stream construction and look-up-table expansion as pmx_expand_kernel, with
// the flip applied while the stream is built (rows bit-reversed, x -> W-1-x).
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t flip_row(uint32_t v, int W, bool flip) { return flip ? (__builtin_bitreverse32(v) >> (32 - W)) : v; }

// One wavefront per ENV.  The two learners' streams are assembled side by side, one per half of the wave (lanes 0-31: the
// first learner's snapshot, lanes 32-63: the second's; H <= 32 rows each), and the merged slot is the first learner's
// stream patched in registers while it is expanded (the ally bit of plane 4 cleared, the mate's bit of plane 1 set), so no
// third stream is built.  The 16-byte vectors of all slots are then dealt to the lanes as ONE index range (2 or 3 x n_vec):
// on smallCapture 231 vectors fill four store instructions to 90 % where one wave per (env, slot) -- the round-2 kernel --
// filled six to 60 %, and the set-up (snapshot loads, stream assembly, the block's look-up table) is paid once per env
// instead of once per slot: 28.3 -> 14.5 us at 16 384 smallCapture envs, 12.3 -> 10.0 / 20.3 -> 17.0 us on the 20 x 20 boards
// (4 096 / 8 192 envs).  U = store instructions per group of look-ups (1: 16.0 us, 2: 14.5, 4: 14.4, 5: 15.0 on smallCapture).
// MIXED (pmx_emit_team_obs_mixed): the colour is the ENV's (p.team_red[env], read once per wave, so first / second / flip stay
// wave-uniform) and the launch covers the envs p.first .. p.first + p.count - 1, output row j = env p.first + j.  The uniform
// instantiation reads none of the three fields and is the kernel it was before they existed.
// FOG (pmx_emit_team_obs_fog / _mixed_fog): the contest's sight rule (capture.py:285-291) on the learners' slots.  An enemy whose
// Manhattan distance to BOTH team agents, in the snapshot of the half that encodes it, exceeds p.sight is left out of that half's
// stream; the merged slot stays full-information, so the first half's hidden enemies (at most two bit offsets, wave-uniform) are
// put back in registers while slot 2 is expanded, as the mate's bit is.  Everything is under `if constexpr (FOG)`: the six
// instantiations without it read no new field and are the code they were.
// BELIEF (pmx_emit_team_obs_belief / _mixed_belief, never together with FOG): learner slot j's plane 5 is the OR of the tracker's two
// sets of that slot (p.belief, row words, x-flipped like every other row) in place of the enemies' point bits; each half ORs its
// 2 x H row words into its own stream.  The merged slot is expanded from the first half's stream and must keep the TRUE enemy
// bits, so its plane 5 is patched in registers: the bits of a vector that fall into [5 HW, 6 HW) are cleared and the first half's
// two enemy offsets (wave-uniform, as FOG's are) are set.  A third, plane-5-only stream in LDS was the alternative; the patch is a
// handful of VALU operations on the merged slot's vectors only and needs no LDS.  Measured with the patch, 16 384 smallCapture envs,
// byte planes, 520 interleaved launches: 15.49 us against 15.33 us for the fog kernel in the same process (profiles/belief).
// Everything is under `if constexpr (BELIEF)`: the twelve instantiations without it read no new field.
// WEIGHTED (pmx_emit_team_obs_weighted / _mixed_weighted, never together with FOG or BELIEF): learner slot j's plane 5 holds the
// weighted tracker's levels (p.levels, one byte per cell, 0 .. 16) as NUMBERS, which a one-bit-per-cell stream cannot carry.  Each
// half stages its HW level bytes x-flipped in LDS (1 KB per half) and puts no bit for plane 5 into its stream; while slots 0 and 1
// are expanded the elements of a vector whose index falls into [5 HW, 6 HW) take the staged bytes, converted to the element type.
// The bytes are staged at offset (5 HW) & 15 with zeroed bytes before and after them, so the 16 / 8 / 4 levels of a vector are ONE
// aligned LDS read at a multiple of the vector's element offset, and they are OR-ed in: the stream has left those elements 0, and
// the zero bytes beside the plane leave the neighbouring planes' elements alone, so no element is tested.  The merged slot takes the first half's stream, which has no plane-5 bit, and gets the two true enemy offsets set
// in registers as BELIEF does.  Everything is under `if constexpr (WEIGHTED)`: the eighteen other instantiations read no new field
// and allocate no new LDS.
#define EMIT_LEVEL_STRIDE 1056          // 1024 level bytes, up to 15 bytes of offset before them and up to 16 zero bytes after
template <bool ON> struct EmitLevelStage { static __device__ __forceinline__ uint8_t *get() { return nullptr; } };
template <> struct EmitLevelStage<true> {
    // [wave][half][16 + cell + 16]
    static __device__ __forceinline__ uint8_t *get() { __shared__ __align__(16) uint8_t stage[4 * 2 * EMIT_LEVEL_STRIDE]; return stage; }
};

// OR the VEC staged level bytes at byte offset `o` of a half's stage (a multiple of VEC) into the vector, as numbers in the
// element type; a zero byte changes nothing (0.0 has no bit set in float32 or bfloat16)
template <int DT>
__device__ __forceinline__ void or_levels(uint4 &v, const uint8_t *LS, int o)
{
    uint32_t *w = reinterpret_cast<uint32_t *>(&v);
    if constexpr (DT == 2) {
        const uint4 r = *reinterpret_cast<const uint4 *>(LS + o);
        v.x |= r.x; v.y |= r.y; v.z |= r.z; v.w |= r.w;
    } else if constexpr (DT == 1) {
        const uint2 r = *reinterpret_cast<const uint2 *>(LS + o);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t byte = ((i < 4 ? r.x : r.y) >> (8 * (i & 3))) & 0xFFu;
            w[i >> 1] |= (__float_as_uint((float)byte) >> 16) << (16 * (i & 1));      // exact in bfloat16: 0 .. 16
        }
    } else {
        const uint32_t r = *reinterpret_cast<const uint32_t *>(LS + o);
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] |= __float_as_uint((float)((r >> (8 * i)) & 0xFFu));
    }
}

template <int DT, bool MIXED, bool FOG, bool BELIEF = false, bool WEIGHTED = false>
__global__ __launch_bounds__(PMX_BLOCK) void pmx_emit_team_kernel(PmxEmitParams p)
{
    constexpr int VEC = ObsVec<DT>::VEC;
    constexpr int U = 2;
    constexpr int TW = 8 * 32 * 32 / 32 + 8;
    __shared__ uint32_t tab[4][2][TW];                        // [wave][learner][stream words]
    __shared__ __align__(16) uint32_t lut[DT == 0 ? 16 * 4 : (DT == 1 ? 256 * 4 : 256 * 2)];
    {
        const uint32_t i = threadIdx.x;
        if (DT == 0) {
            if (i < 16) *reinterpret_cast<uint4 *>(&lut[4 * i]) = pack_obs<0>(i);
        } else if (DT == 1) {
            *reinterpret_cast<uint4 *>(&lut[4 * i]) = pack_obs<1>(i);
        } else {
            lut[2 * i] = ((i & 15u) * 0x00204081u) & 0x01010101u;
            lut[2 * i + 1] = ((i >> 4) * 0x00204081u) & 0x01010101u;
        }
        __syncthreads();
    }
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int half = lane >> 5, hl = lane & 31;
    const int W = p.lay_W, H = p.lay_H, HW = H * W;
    long blk = (long)blockIdx.x;
    if (((MIXED ? p.count : p.N) & 127) == 0) {               // the 16 envs of one 64-byte line of snapshot words: one XCD
        const long r = blk & 31;                              // (a permutation of the launched blocks: whole groups of 32 only)
        blk = (blk & ~31L) + (r & 7) * 4 + (r >> 3);
    }
    const long row = blk * 4 + wave;                          // output row; the env itself unless MIXED
    if (row >= (MIXED ? p.count : p.N)) return;
    const long env = MIXED ? row + p.first : row;
    const int red_v = MIXED ? __builtin_amdgcn_readfirstlane((int)p.team_red[env]) : p.red;
    const bool flip = red_v != 0;
    const int first = red_v ? 0 : 1, second = first + 2;
    const int agent = half ? second : first;
    const size_t N = (size_t)p.N;
    const uint32_t *S = (MIXED ? (half ? (flip ? p.snap[2] : p.snap[3]) : (flip ? p.snap[0] : p.snap[1]))
                               : (half ? p.snap[second] : p.snap[first])) + env;
    uint32_t *T = tab[wave][half];
    const PmxLayoutDev *L = p.lay + (p.layout_idx ? p.layout_idx[env] : 0);

    const uint32_t food = hl < H ? S[(size_t)hl * N] : 0u;
    [[maybe_unused]] uint32_t bel = 0;                        // BELIEF: row hl of this slot's two sets, OR-ed
    if constexpr (BELIEF) {
        if (hl < H) {
            const uint32_t *B = p.belief + ((size_t)row * 4 + (size_t)half * 2) * 32 + hl;
            bel = B[0] | B[32];
        }
    }
    uint32_t pt = 0;
    if (hl < 4) pt = S[(size_t)PMX_W_AGENT_A(H, hl) * N];
    else if (hl < 8) pt = S[(size_t)PMX_W_CAPS(H, (hl - 4) >> 1) * N];
    const uint32_t a_self = S[(size_t)PMX_W_AGENT_A(H, agent) * N];
    const uint32_t b_self = S[(size_t)PMX_W_AGENT_B(H, agent) * N];
    const int n_words = (8 * HW + 31) >> 5;
    const int wall_words = (HW + 31) >> 5;
    for (int k = hl; k < n_words + 1; k += 32) T[k] = (!flip && k < wall_words) ? L->wall_stream[k] : 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (hl < H) {
        if (flip) stream_or_row(T, (uint32_t)(hl * W), flip_row(L->walls[hl], W, true), W);
        const uint32_t blue = flip_row(food & L->hi_mask, W, flip), red = flip_row(food & L->lo_mask, W, flip);
        stream_or_row(T, (uint32_t)(((flip ? 7 : 6) * H + hl) * W), blue, W);
        stream_or_row(T, (uint32_t)(((flip ? 6 : 7) * H + hl) * W), red, W);
        if constexpr (BELIEF) stream_or_row(T, (uint32_t)((5 * H + hl) * W), flip_row(bel, W, flip), W);
    }
    if constexpr (WEIGHTED) {                                 // this half's levels, x-flipped like every row; c / W by a reciprocal
        uint8_t *LS = EmitLevelStage<WEIGHTED>::get() + (wave * 2 + half) * EMIT_LEVEL_STRIDE;     // (exact for c < 1055, W <= 32)
        const uint8_t *G = p.levels + ((size_t)row * 2 + half) * HW;
        const int inv = (65536 + W - 1) / W, pad = (5 * HW) & 15;
        // zero the 16 bytes the levels begin in and the 16 they end in (LDS stores of a wave are in order: the bytes come after)
        if (hl < 4) reinterpret_cast<uint32_t *>(LS)[hl] = 0u;
        else if (hl < 8) reinterpret_cast<uint32_t *>(LS + ((pad + HW) & ~15))[hl - 4] = 0u;
        for (int c = hl; c < HW; c += 32) {
            const int yc = (c * inv) >> 16, xc = c - yc * W;
            LS[pad + (flip ? yc * W + (W - 1 - xc) : c)] = G[c];
        }
    }
    uint32_t pt_off = 0;                                      // lanes 0-3 of each half: that agent's bit offset in the stream
    [[maybe_unused]] int hid_v = -1;                          // FOG, lanes 0-3 of each half: pt_off of an enemy this half does not see
    [[maybe_unused]] uint32_t team_a = 0, team_b = 0;         // FOG: word A of the two team agents in this half's snapshot
    if constexpr (FOG) {
        const int a0 = first ? __builtin_amdgcn_readlane((int)pt, 1) : __builtin_amdgcn_readlane((int)pt, 0);
        const int b0 = first ? __builtin_amdgcn_readlane((int)pt, 3) : __builtin_amdgcn_readlane((int)pt, 2);
        const int a1 = first ? __builtin_amdgcn_readlane((int)pt, 33) : __builtin_amdgcn_readlane((int)pt, 32);
        const int b1 = first ? __builtin_amdgcn_readlane((int)pt, 35) : __builtin_amdgcn_readlane((int)pt, 34);
        team_a = (uint32_t)(half ? a1 : a0), team_b = (uint32_t)(half ? b1 : b0);
    }
    if (hl < 4) {
        const int x0 = pt & 0xFF, y = (pt >> 8) & 0xFF, x = flip ? W - 1 - x0 : x0;
        const int plane = hl == agent ? 1 : (((hl ^ agent) == 2) ? 4 : 5);
        pt_off = (uint32_t)((plane * H + y) * W + x);
        bool shown = true;
        if constexpr (FOG) {                                  // the x-flip keeps |dx|, so the snapshot's own coordinates serve
            const int da = abs(x0 - (int)(team_a & 0xFF)) + abs(y - (int)((team_a >> 8) & 0xFF));
            const int db = abs(x0 - (int)(team_b & 0xFF)) + abs(y - (int)((team_b >> 8) & 0xFF));
            shown = plane != 5 || (da < db ? da : db) <= p.sight;
            if (!shown) hid_v = (int)pt_off;
        }
        if constexpr (BELIEF || WEIGHTED) shown = plane != 5;   // the sets / the levels stand in for the enemies' own bits
        if (shown) atomicOr(&T[pt_off >> 5], 1u << (pt_off & 31));
    } else if (hl < 8) {
        const uint32_t cxy = (pt >> (16 * ((hl - 4) & 1))) & 0xFFFFu;
        if (cxy != 0xFFFFu) {
            const int x0 = cxy & 0xFF, y = cxy >> 8, x = flip ? W - 1 - x0 : x0;
            const int plane0 = (2 * x0 > W) ? 2 : 3;
            const int plane = flip ? 5 - plane0 : plane0;
            const uint32_t off = (uint32_t)((plane * H + y) * W + x);
            atomicOr(&T[off >> 5], 1u << (off & 31));
        }
    }
    const int sx = (int)(a_self & 0xFF);
    const int fself_v = (H + (int)((a_self >> 8) & 0xFF)) * W + (flip ? W - 1 - sx : sx);
    const int fself0 = __builtin_amdgcn_readlane(fself_v, 0), fself1 = __builtin_amdgcn_readlane(fself_v, 32);
    const uint32_t carry0 = (__builtin_amdgcn_readlane((int)b_self, 0) >> 8) & 0xFFF;
    const uint32_t carry1 = (__builtin_amdgcn_readlane((int)b_self, 32) >> 8) & 0xFFF;
    // merged slot (merge_obs_for_critic): plane 4 of the first learner's stream cleared, the second learner -- where ITS OWN
    // snapshot has it -- added to plane 1; both learners on one cell: max(1 + carry, 1 + carry')
    const int f_ally = second == 2 ? __builtin_amdgcn_readlane((int)pt_off, 2) : __builtin_amdgcn_readlane((int)pt_off, 3);
    int fmate = fself1;
    uint32_t carry_m = carry0;
    if (fmate == fself0) {
        carry_m = carry0 > carry1 ? carry0 : carry1;
        fmate = -1;
    }
    // FOG: the first half's hidden enemies (its lanes 1 - first and 3 - first), -1 = seen; two on one cell share their distances
    [[maybe_unused]] int hid_a = -1, hid_b = -1;
    if constexpr (FOG) {
        hid_a = first ? __builtin_amdgcn_readlane(hid_v, 0) : __builtin_amdgcn_readlane(hid_v, 1);
        hid_b = first ? __builtin_amdgcn_readlane(hid_v, 2) : __builtin_amdgcn_readlane(hid_v, 3);
    }
    // BELIEF: the first half's two enemy offsets, which the merged slot gets back in place of that half's sets
    [[maybe_unused]] int en_a = -1, en_b = -1;
    if constexpr (BELIEF || WEIGHTED) {
        en_a = first ? __builtin_amdgcn_readlane((int)pt_off, 0) : __builtin_amdgcn_readlane((int)pt_off, 1);
        en_b = first ? __builtin_amdgcn_readlane((int)pt_off, 2) : __builtin_amdgcn_readlane((int)pt_off, 3);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    const int n_vec = 8 * HW / VEC;
    const int total = (p.merged ? 3 : 2) * n_vec;
    uint4 *out_team = reinterpret_cast<uint4 *>(p.team_obs) + (size_t)row * 2 * n_vec;            // slots 0, 1 are contiguous
    uint4 *out_merged = reinterpret_cast<uint4 *>(p.merged) + (size_t)row * n_vec - 2 * n_vec;   // indexed by kk >= 2 n_vec
    const uint32_t *T0 = tab[wave][0], *T1 = tab[wave][1];
    for (int base = 0; base < total; base += 64 * U) {
        uint32_t bits[U], e0s[U];
        int sl[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kk = base + 64 * u + lane;
            const int s = (kk >= n_vec) + (kk >= 2 * n_vec);
            const bool ok = kk < total;
            sl[u] = ok ? s : 0;
            e0s[u] = ok ? (uint32_t)(kk - s * n_vec) * VEC : 0u;
            bits[u] = (sl[u] == 1 ? T1 : T0)[e0s[u] >> 5] >> (e0s[u] & 31);
            if (sl[u] == 2) {
                const uint32_t d4 = (uint32_t)(f_ally - (int)e0s[u]);
                if (d4 < (uint32_t)VEC) bits[u] &= ~(1u << d4);
                const uint32_t d2 = (uint32_t)(fmate - (int)e0s[u]);
                if (fmate >= 0 && d2 < (uint32_t)VEC) bits[u] |= 1u << d2;
                if constexpr (FOG) {                          // nothing is hidden from the critic (-1 - e0 is no offset below VEC)
                    const uint32_t ha = (uint32_t)(hid_a - (int)e0s[u]), hb = (uint32_t)(hid_b - (int)e0s[u]);
                    if (ha < (uint32_t)VEC) bits[u] |= 1u << ha;
                    if (hb < (uint32_t)VEC) bits[u] |= 1u << hb;
                }
                if constexpr (BELIEF) {                       // plane 5 of the critic's input: the true enemies, not the sets
                    const int lo = 5 * HW - (int)e0s[u], hi = 6 * HW - (int)e0s[u];
                    if (lo < VEC && hi > 0) {
                        const uint32_t below_hi = hi >= VEC ? (1u << VEC) - 1u : (1u << hi) - 1u;
                        bits[u] &= ~(below_hi & ~(lo > 0 ? (1u << lo) - 1u : 0u));
                    }
                    const uint32_t ea = (uint32_t)(en_a - (int)e0s[u]), eb = (uint32_t)(en_b - (int)e0s[u]);
                    if (ea < (uint32_t)VEC) bits[u] |= 1u << ea;
                    if (eb < (uint32_t)VEC) bits[u] |= 1u << eb;
                }
                if constexpr (WEIGHTED) {                     // the first half's stream has no plane-5 bit: the true enemies go in
                    const uint32_t ea = (uint32_t)(en_a - (int)e0s[u]), eb = (uint32_t)(en_b - (int)e0s[u]);
                    if (ea < (uint32_t)VEC) bits[u] |= 1u << ea;
                    if (eb < (uint32_t)VEC) bits[u] |= 1u << eb;
                }
            }
        }
        uint4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (DT == 0) v[u] = *reinterpret_cast<const uint4 *>(&lut[(bits[u] & 15u) * 4]);
            else if (DT == 1) v[u] = *reinterpret_cast<const uint4 *>(&lut[(bits[u] & 255u) * 4]);
            else {
                const uint2 lo = *reinterpret_cast<const uint2 *>(&lut[(bits[u] & 255u) * 2]);
                const uint2 hi = *reinterpret_cast<const uint2 *>(&lut[((bits[u] >> 8) & 255u) * 2]);
                v[u] = make_uint4(lo.x, lo.y, hi.x, hi.y);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kk = base + 64 * u + lane;
            const int fs = sl[u] == 1 ? fself1 : fself0;
            const uint32_t cr = sl[u] == 0 ? carry0 : (sl[u] == 1 ? carry1 : carry_m);
            const uint32_t d = (uint32_t)(fs - (int)e0s[u]);
            if (d < (uint32_t)VEC) patch_self<DT>(v[u], (int)d, cr);
            if (sl[u] == 2 && fmate >= 0) {
                const uint32_t d2 = (uint32_t)(fmate - (int)e0s[u]);
                if (d2 < (uint32_t)VEC) patch_self<DT>(v[u], (int)d2, carry1);
            }
            if constexpr (WEIGHTED) {                         // slots 0 and 1: plane 5 is the staged levels, as numbers
                const int lo = 5 * HW - (int)e0s[u];          // the vector holds cells -lo .. VEC - 1 - lo of plane 5
                if (kk < 2 * n_vec && lo < VEC && lo + HW > 0)
                    or_levels<DT>(v[u], EmitLevelStage<WEIGHTED>::get() + (wave * 2 + sl[u]) * EMIT_LEVEL_STRIDE, ((5 * HW) & 15) - lo);
            }
            if (kk < total) (sl[u] == 2 ? out_merged : out_team)[kk] = v[u];
        }
    }
}

// ev0 / ev1 (both or neither): start / stop events of this very dispatch, as in pmx_launch_expand
extern "C" hipError_t pmx_launch_emit_team(const PmxEmitParams *p, int dtype, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
{
    const unsigned blocks = (unsigned)(((long)p->N + 3) / 4);    // one wave per env
#define PMX_EMIT(DT, MIXED, FOG)                                                                                                   \
    do {                                                                                                                           \
        if (ev0) hipExtLaunchKernelGGL((pmx_emit_team_kernel<DT, MIXED, FOG>), dim3(blocks), dim3(PMX_BLOCK), 0, st, ev0, ev1, 0, *p); \
        else hipLaunchKernelGGL((pmx_emit_team_kernel<DT, MIXED, FOG>), dim3(blocks), dim3(PMX_BLOCK), 0, st, *p);                  \
    } while (0)
    switch (dtype) {
    case 0: PMX_EMIT(0, false, false); break;
    case 1: PMX_EMIT(1, false, false); break;
    default: PMX_EMIT(2, false, false); break;
    }
    return hipGetLastError();
}

// pmx_emit_team_obs_fog / pmx_emit_team_obs_mixed_fog: p->sight set; mixed != 0: the fields of pmx_launch_emit_team_mixed too
extern "C" hipError_t pmx_launch_emit_team_fog(const PmxEmitParams *p, int mixed, int dtype, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
{
    const unsigned blocks = (unsigned)(((long)(mixed ? p->count : p->N) + 3) / 4);
    switch (dtype + (mixed ? 3 : 0)) {
    case 0: PMX_EMIT(0, false, true); break;
    case 1: PMX_EMIT(1, false, true); break;
    case 2: PMX_EMIT(2, false, true); break;
    case 3: PMX_EMIT(0, true, true); break;
    case 4: PMX_EMIT(1, true, true); break;
    default: PMX_EMIT(2, true, true); break;
    }
    return hipGetLastError();
}

// pmx_emit_team_obs_mixed: p->team_red, p->first and p->count set, one wave per env of the range (p->count > 0)
extern "C" hipError_t pmx_launch_emit_team_mixed(const PmxEmitParams *p, int dtype, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
{
    const unsigned blocks = (unsigned)(((long)p->count + 3) / 4);
    switch (dtype) {
    case 0: PMX_EMIT(0, true, false); break;
    case 1: PMX_EMIT(1, true, false); break;
    default: PMX_EMIT(2, true, false); break;
    }
    return hipGetLastError();
}

// pmx_emit_team_obs_belief / pmx_emit_team_obs_mixed_belief: p->belief set; mixed != 0: the fields of pmx_launch_emit_team_mixed too
extern "C" hipError_t pmx_launch_emit_team_belief(const PmxEmitParams *p, int mixed, int dtype, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
{
    const unsigned blocks = (unsigned)(((long)(mixed ? p->count : p->N) + 3) / 4);
#define PMX_EMIT_BELIEF(DT, MIXED)                                                                                                 \
    do {                                                                                                                           \
        if (ev0) hipExtLaunchKernelGGL((pmx_emit_team_kernel<DT, MIXED, false, true>), dim3(blocks), dim3(PMX_BLOCK), 0, st, ev0, ev1, 0, *p); \
        else hipLaunchKernelGGL((pmx_emit_team_kernel<DT, MIXED, false, true>), dim3(blocks), dim3(PMX_BLOCK), 0, st, *p);          \
    } while (0)
    switch (dtype + (mixed ? 3 : 0)) {
    case 0: PMX_EMIT_BELIEF(0, false); break;
    case 1: PMX_EMIT_BELIEF(1, false); break;
    case 2: PMX_EMIT_BELIEF(2, false); break;
    case 3: PMX_EMIT_BELIEF(0, true); break;
    case 4: PMX_EMIT_BELIEF(1, true); break;
    default: PMX_EMIT_BELIEF(2, true); break;
    }
#undef PMX_EMIT_BELIEF
#undef PMX_EMIT
    return hipGetLastError();
}

// pmx_emit_team_obs_weighted / pmx_emit_team_obs_mixed_weighted: p->levels set; mixed != 0: the fields of pmx_launch_emit_team_mixed too
extern "C" hipError_t pmx_launch_emit_team_weighted(const PmxEmitParams *p, int mixed, int dtype, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
{
    const unsigned blocks = (unsigned)(((long)(mixed ? p->count : p->N) + 3) / 4);
#define PMX_EMIT_WEIGHTED(DT, MIXED)                                                                                               \
    do {                                                                                                                           \
        if (ev0) hipExtLaunchKernelGGL((pmx_emit_team_kernel<DT, MIXED, false, false, true>), dim3(blocks), dim3(PMX_BLOCK), 0, st, ev0, ev1, 0, *p); \
        else hipLaunchKernelGGL((pmx_emit_team_kernel<DT, MIXED, false, false, true>), dim3(blocks), dim3(PMX_BLOCK), 0, st, *p);   \
    } while (0)
    switch (dtype + (mixed ? 3 : 0)) {
    case 0: PMX_EMIT_WEIGHTED(0, false); break;
    case 1: PMX_EMIT_WEIGHTED(1, false); break;
    case 2: PMX_EMIT_WEIGHTED(2, false); break;
    case 3: PMX_EMIT_WEIGHTED(0, true); break;
    case 4: PMX_EMIT_WEIGHTED(1, true); break;
    default: PMX_EMIT_WEIGHTED(2, true); break;
    }
#undef PMX_EMIT_WEIGHTED
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// Belief sets and weights of the hidden enemies: the kernels are in pmx_belief.h; here the launchers of the forms without evidence
// ---------------------------------------------------------------------------------------------------------------
// count > 0 rows, one wave each; ev0 / ev1 as in pmx_launch_emit_team (the update kernel only)
extern "C" hipError_t pmx_launch_belief(const PmxBeliefParams *p, int init, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
{
    const unsigned blocks = (unsigned)(((long)p->count + 3) / 4);
    if (init) hipLaunchKernelGGL(pmx_belief_kernel<true>, dim3(blocks), dim3(PMX_BLOCK), 0, st, *p, BeliefEvidenceArg<false>{});
    else if (ev0) hipExtLaunchKernelGGL(pmx_belief_kernel<false>, dim3(blocks), dim3(PMX_BLOCK), 0, st, ev0, ev1, 0, *p, BeliefEvidenceArg<false>{});
    else hipLaunchKernelGGL(pmx_belief_kernel<false>, dim3(blocks), dim3(PMX_BLOCK), 0, st, *p, BeliefEvidenceArg<false>{});
    return hipGetLastError();
}

// count > 0 rows, one wave each; ev0 / ev1 as in pmx_launch_belief (the update kernel only)
extern "C" hipError_t pmx_launch_belief_weights(const PmxBeliefWeightsParams *p, int init, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
{
    const unsigned blocks = (unsigned)(((long)p->b.count + 3) / 4);
    if (init) hipLaunchKernelGGL(pmx_belief_weights_kernel<true>, dim3(blocks), dim3(PMX_BLOCK), 0, st, *p, BeliefEvidenceArg<false>{});
    else if (ev0) hipExtLaunchKernelGGL(pmx_belief_weights_kernel<false>, dim3(blocks), dim3(PMX_BLOCK), 0, st, ev0, ev1, 0, *p, BeliefEvidenceArg<false>{});
    else hipLaunchKernelGGL(pmx_belief_weights_kernel<false>, dim3(blocks), dim3(PMX_BLOCK), 0, st, *p, BeliefEvidenceArg<false>{});
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// host-side launchers (called by the C ABI in pmx_api.hip)
// ---------------------------------------------------------------------------------------------------------------
// ev0/ev1 (both or neither): events that receive the START and STOP timestamps of this very dispatch (hipExtLaunchKernelGGL),
// i.e. the kernel's own duration as a profiler sees it, without the dispatch gaps a hipEventRecord pair would include
extern "C" hipError_t pmx_launch_rule(const PmxTickParams *p, int H, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
{
    const int rule_blocks = (p->N + PMX_RULE_BLOCK - 1) / PMX_RULE_BLOCK;
    const size_t lds = (p->layout_idx ? 32 + (size_t)(3 * PMX_MAX_H_LDS + 32 + 16) * PMX_RULE_BLOCK : 32 + (size_t)(3 * H + 16) * PMX_RULE_BLOCK) * sizeof(uint32_t);
    // row loops unrolled for the board-height bucket (see load_env_issue)
    const int hb = H <= 12 ? 12 : (H <= 16 ? 16 : (H <= 20 ? 20 : 32));
    // p->obs: the wall writer's blocks follow the rule blocks, which keep the low block ids and so are dispatched first.  A
    // wall block is one wave and carries the same dynamic LDS reservation as a rule block (9.6 KB for smallCapture, 37 KB
    // with per-env layouts), of which it uses nothing: PMX_WALL_BLOCKS = 4 per CU stays inside the 160 KB of a CU
    // next to the CU's rule block in the first case, and queues behind it in the second.
    // Block counts and store policies measured, and why float32 planes only: profiles/wall_split/README.md.
    const long obs_blocks = (long)p->N * p->n_emit;
    const int wall_blocks = p->obs ? (int)std::min<long>(obs_blocks, PMX_WALL_BLOCKS) : 0;
    const int blocks = rule_blocks + wall_blocks;
    PmxTickParams q = *p;
    q.rule_blocks = rule_blocks;
#define PMX_RULE_LAUNCH(B, HBV)                                                                                         \
    do {                                                                                                                \
        if (ev0) hipExtLaunchKernelGGL((pmx_rule_kernel<B, HBV>), dim3(blocks), dim3(PMX_RULE_BLOCK), (uint32_t)lds, st, ev0, ev1, 0, q); \
        else hipLaunchKernelGGL((pmx_rule_kernel<B, HBV>), dim3(blocks), dim3(PMX_RULE_BLOCK), lds, st, q);               \
    } while (0)
#define PMX_RULE_PICK(B)                                                                      \
    switch (hb) {                                                                             \
    case 12: PMX_RULE_LAUNCH(B, 12); break;                                                   \
    case 16: PMX_RULE_LAUNCH(B, 16); break;                                                   \
    case 20: PMX_RULE_LAUNCH(B, 20); break;                                                   \
    default: PMX_RULE_LAUNCH(B, 32); break;                                                   \
    }
    if (p->dist && p->bot_sight > 0) {      // the sight form of the bots variant (pmx_set_bot_sight)
        switch (hb) {
#define PMX_RULE_SIGHT_LAUNCH(HBV)                                                                                       \
    do {                                                                                                                \
        if (ev0) hipExtLaunchKernelGGL((pmx_rule_sight_kernel<HBV>), dim3(blocks), dim3(PMX_RULE_BLOCK), (uint32_t)lds, st, ev0, ev1, 0, q); \
        else hipLaunchKernelGGL((pmx_rule_sight_kernel<HBV>), dim3(blocks), dim3(PMX_RULE_BLOCK), lds, st, q);            \
    } while (0)
        case 12: PMX_RULE_SIGHT_LAUNCH(12); break;
        case 16: PMX_RULE_SIGHT_LAUNCH(16); break;
        case 20: PMX_RULE_SIGHT_LAUNCH(20); break;
        default: PMX_RULE_SIGHT_LAUNCH(32); break;
        }
    } else if (p->dist) { PMX_RULE_PICK(true) } else { PMX_RULE_PICK(false) }
    return hipGetLastError();
}

// The fused tick (pmx_tick_fused_kernel): N / 64 workgroups of 16 waves.  The caller (pmx_step) has checked what the kernel
// assumes: float32 planes of all four agents, one layout, no bots, H <= 20, N % 64 == 0.  With H <= 20 and W <= 32 the LDS
// request is at most 61 952 bytes, inside the 64 KB a launch may ask for without a function attribute.
extern "C" hipError_t pmx_launch_tick_fused(const PmxTickParams *p, int reverse, hipStream_t st)
{
    const int H = p->lay_H, W = p->lay_W;
    if (H > 20 || (p->N % PMX_RULE_BLOCK) != 0 || p->layout_idx || p->dist || !p->obs || p->n_emit != 4) return hipErrorInvalidValue;
    const size_t lds = ((size_t)fused_rule_words(H) + (size_t)fused_snap_rows(H) * PMX_RULE_BLOCK + 64 + 32 + 4 +
                        (size_t)PMX_FUSED_WAVES * fused_tab_stride(H, W)) * sizeof(uint32_t);
    if (lds > ((size_t)64 << 10)) return hipErrorInvalidValue;
    const dim3 grid(p->N / PMX_RULE_BLOCK), block(PMX_FUSED_WAVES * 64);
    if (H <= 12) hipLaunchKernelGGL(pmx_tick_fused_kernel<12>, grid, block, lds, st, *p, reverse);
    else if (H <= 16) hipLaunchKernelGGL(pmx_tick_fused_kernel<16>, grid, block, lds, st, *p, reverse);
    else hipLaunchKernelGGL(pmx_tick_fused_kernel<20>, grid, block, lds, st, *p, reverse);
    return hipGetLastError();
}

extern "C" hipError_t pmx_launch_rule_agent(const PmxTickParams *p, int H, int agent, hipStream_t st)
{
    const int blocks = (p->N + PMX_RULE_BLOCK - 1) / PMX_RULE_BLOCK;
    const size_t lds = (p->layout_idx ? 32 + (size_t)(3 * PMX_MAX_H_LDS + 32 + 16) * PMX_RULE_BLOCK : 32 + (size_t)(3 * H + 16) * PMX_RULE_BLOCK) * sizeof(uint32_t);
    if (p->dist && p->bot_sight > 0) hipLaunchKernelGGL(pmx_rule_agent_sight_kernel, dim3(blocks), dim3(PMX_RULE_BLOCK), lds, st, *p, agent);
    else if (p->dist) hipLaunchKernelGGL(pmx_rule_agent_kernel<true>, dim3(blocks), dim3(PMX_RULE_BLOCK), lds, st, *p, agent);
    else hipLaunchKernelGGL(pmx_rule_agent_kernel<false>, dim3(blocks), dim3(PMX_RULE_BLOCK), lds, st, *p, agent);
    return hipGetLastError();
}

extern "C" hipError_t pmx_launch_successor(const PmxTickParams *p, int H, int agent, hipStream_t st)
{
    const int blocks = (p->N + PMX_RULE_BLOCK - 1) / PMX_RULE_BLOCK;
    const size_t lds = (p->layout_idx ? 32 + (size_t)(3 * PMX_MAX_H_LDS + 32 + 16) * PMX_RULE_BLOCK : 32 + (size_t)(3 * H + 16) * PMX_RULE_BLOCK) * sizeof(uint32_t);
    hipLaunchKernelGGL(pmx_successor_kernel, dim3(blocks), dim3(PMX_RULE_BLOCK), lds, st, *p, agent);
    return hipGetLastError();
}

extern "C" hipError_t pmx_launch_bot_query(const PmxTickParams *p, int H, int agent, int code, double *values, int8_t *action,
                                           uint8_t *flags, hipStream_t st)
{
    const int blocks = (p->N + PMX_RULE_BLOCK - 1) / PMX_RULE_BLOCK;
    const size_t lds = (p->layout_idx ? 32 + (size_t)(3 * PMX_MAX_H_LDS + 32 + 16) * PMX_RULE_BLOCK : 32 + (size_t)(3 * H + 16) * PMX_RULE_BLOCK) * sizeof(uint32_t);
    if (p->dist && p->bot_sight > 0)
        hipLaunchKernelGGL(pmx_bot_query_sight_kernel, dim3(blocks), dim3(PMX_RULE_BLOCK), lds, st, *p, agent, code, values, action, flags);
    else hipLaunchKernelGGL(pmx_bot_query_kernel, dim3(blocks), dim3(PMX_RULE_BLOCK), lds, st, *p, agent, code, values, action, flags);
    return hipGetLastError();
}

extern "C" hipError_t pmx_launch_reset(const PmxTickParams *p, int H, hipStream_t st)
{
    const int blocks = (p->N + PMX_RULE_BLOCK - 1) / PMX_RULE_BLOCK;
    const size_t lds = (p->layout_idx ? 32 + (size_t)(3 * PMX_MAX_H_LDS + 32 + 16) * PMX_RULE_BLOCK : 32 + (size_t)(3 * H + 16) * PMX_RULE_BLOCK) * sizeof(uint32_t);
    hipLaunchKernelGGL(pmx_reset_kernel, dim3(blocks), dim3(PMX_RULE_BLOCK), lds, st, *p);
    return hipGetLastError();
}

extern "C" hipError_t pmx_launch_expand(const PmxExpandParams *p, int dtype, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
{
    const long waves = (long)p->N * p->n_emit;
    const unsigned blocks = (unsigned)((waves + 3) / 4);
    // Store policy, measured in one process (us per launch):
    //   f32   323 MB  ordinary 53.7 | nt 64.9 | nt + 3 blocks/CU 60.0
    //         646 MB  ordinary 114.6 | nt 126.1 | nt + 3 blocks/CU 107.2
    //        1.29 GB  ordinary 262 | nt 246 | nt + 4 blocks/CU 227 | nt + 3 blocks/CU 207.8 | nt + 2 blocks/CU 278
    //   bf16  161 MB  31.6/35.9   323 MB 61.1/66.7  646 MB 172/124 (ordinary / nt)
    //   u8     80 MB  29.6/28.5   323 MB 111/102
    // Ordinary stores win while the 256 MiB Infinity Cache can absorb a good part of the planes.  Beyond that, streaming
    // (non-temporal) stores win, and they win more with FEWER wavefronts in flight: every wave is its own sequential
    // write stream, and 12 waves per CU instead of 32 keep the number of DRAM pages open at once low enough for the
    // write-combined bursts to stay row-buffer hits (6.2 TB/s instead of 5.3 at 1.29 GB).  The occupancy cap is an
    // unused dynamic-LDS reservation of 40 000 bytes per block (3 blocks of 4 waves fit the 160 KB of a CU).
    // (the cap is for float32 only: the bf16 / uint8 variants are issue-bound and lose up to 2x with it)
    //
    // Alternating sweep: a caller steps the same observation buffer tick after tick, and the last part written in tick t is
    // still in the Infinity Cache when tick t+1 starts.  Walking the blocks in the opposite direction every other tick makes
    // tick t+1 overwrite exactly those lines first, while they are still cached, so they never cost an HBM write:
    //   f32 small 323 MB  51.4 -> 43.8 us      blox 419 MB  75.7 -> 60.4      blox 839 MB  151.8 -> 125.1
    //       small 646 MB 118.7 -> 108.6 (streaming + cap: 105-107)       small 1.29 GB  271 -> 257 (streaming + cap: 208)
    // It needs ordinary (cache-allocating) stores, so float32 planes up to 900 MB now use them; p->reverse carries the parity.
    const size_t elem = dtype == 0 ? 4 : (dtype == 1 ? 2 : 1);
    const size_t bytes = (size_t)waves * 8 * p->lay_H * p->lay_W * elem;
    // uint8 planes always take streaming stores (and so never the alternating sweep); float32 and bfloat16 by size
    const bool nt = elem == 1 || (elem == 2 && bytes > ((size_t)512 << 20)) || (elem == 4 && bytes > PMX_F32_STREAM_BYTES);
    const size_t lds_pad = (nt && elem == 4) ? 40000 : 0;
    PmxExpandParams q = *p;
    if (nt) q.reverse = 0;
    // uint8 planes with all four agents emitted: one wave per env (pmx_expand4_kernel; measured at 16 384 envs of smallCapture:
    // 25.8 -> 22.4 us for uint8, but 26.7 -> 28.3 us for bfloat16, which therefore keeps the wave per (env, agent))
    if (dtype == 2 && p->n_emit == 4 && p->single_agent < 0) {
        const unsigned b4 = (unsigned)((p->N + 3) / 4);
        // this kernel's planes fit the Infinity Cache up to a few hundred MB: ordinary stores there, streaming beyond
        const bool nt4 = bytes > ((size_t)200 << 20);
#define PMX_EXPAND4(NTV)                                                                                                  \
    do {                                                                                                                  \
        if (ev0) hipExtLaunchKernelGGL((pmx_expand4_kernel<NTV>), dim3(b4), dim3(PMX_BLOCK), 0, st, ev0, ev1, 0, q);      \
        else hipLaunchKernelGGL((pmx_expand4_kernel<NTV>), dim3(b4), dim3(PMX_BLOCK), 0, st, q);                          \
    } while (0)
        if (nt4) PMX_EXPAND4(true); else PMX_EXPAND4(false);
#undef PMX_EXPAND4
        return hipGetLastError();
    }
#define PMX_EXPAND(...)                                                                                                 \
    do {                                                                                                                \
        if (ev0) hipExtLaunchKernelGGL((pmx_expand_kernel<__VA_ARGS__>), dim3(blocks), dim3(PMX_BLOCK), (uint32_t)lds_pad, st, ev0, ev1, 0, q); \
        else hipLaunchKernelGGL((pmx_expand_kernel<__VA_ARGS__>), dim3(blocks), dim3(PMX_BLOCK), lds_pad, st, q);       \
    } while (0)
    // first_vec > 0 comes from pmx_step for float32 planes up to PMX_F32_STREAM_BYTES only, i.e. never with nt
    if (q.first_vec > 0 && (dtype != 0 || nt)) return hipErrorInvalidValue;
    switch (dtype) {
    case 0: if (nt) PMX_EXPAND(0, true); else if (q.first_vec > 0) PMX_EXPAND(0, false, true); else PMX_EXPAND(0, false); break;
    case 1: if (nt) PMX_EXPAND(1, true); else PMX_EXPAND(1, false); break;
    default: PMX_EXPAND(2, true); break;
    }
#undef PMX_EXPAND
    return hipGetLastError();
}

// The sight form of the expansion (pmx_set_obs_sight): pmx_launch_expand's grid, store policy and occupancy cap, always the wave
// per (env, agent) kernel (uint8 planes of four agents too) and always the full block (first_vec is refused).
extern "C" hipError_t pmx_launch_expand_sight(const PmxExpandParams *p, int dtype, int sight, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
{
    const long waves = (long)p->N * p->n_emit;
    const unsigned blocks = (unsigned)((waves + 3) / 4);
    const size_t elem = dtype == 0 ? 4 : (dtype == 1 ? 2 : 1);
    const size_t bytes = (size_t)waves * 8 * p->lay_H * p->lay_W * elem;
    const bool nt = elem == 1 || (elem == 2 && bytes > ((size_t)512 << 20)) || (elem == 4 && bytes > PMX_F32_STREAM_BYTES);
    const size_t lds_pad = (nt && elem == 4) ? 40000 : 0;
    PmxExpandParams q = *p;
    if (nt) q.reverse = 0;
    if (q.first_vec > 0) return hipErrorInvalidValue;
#define PMX_EXPAND_SIGHT(...)                                                                                           \
    do {                                                                                                                \
        if (ev0) hipExtLaunchKernelGGL((pmx_expand_sight_kernel<__VA_ARGS__>), dim3(blocks), dim3(PMX_BLOCK), (uint32_t)lds_pad, st, ev0, ev1, 0, q, sight); \
        else hipLaunchKernelGGL((pmx_expand_sight_kernel<__VA_ARGS__>), dim3(blocks), dim3(PMX_BLOCK), lds_pad, st, q, sight); \
    } while (0)
    switch (dtype) {
    case 0: if (nt) PMX_EXPAND_SIGHT(0, true); else PMX_EXPAND_SIGHT(0, false); break;
    case 1: if (nt) PMX_EXPAND_SIGHT(1, true); else PMX_EXPAND_SIGHT(1, false); break;
    default: PMX_EXPAND_SIGHT(2, true); break;
    }
#undef PMX_EXPAND_SIGHT
    return hipGetLastError();
}
