// pmx_belief.h -- the belief trackers' kernels (include/pmx.h, "Belief sets", "Belief weights", "Belief evidence"), gfx950 only.
// A header, because two translation units instantiate them: pmx_step.hip the forms without evidence, pmx_belief_evidence.hip the
// EVIDENCE forms.  In one code object the mere presence of the EVIDENCE instantiations changed the register allocation of
// pmx_belief_weights_kernel<false>; in two, the four existing kernels compile to the instructions they had.
#pragma once
#include <cstdlib>

#include "pmx_device.h"

// The counter-based generator of the bots' draws and the sonar's (include/pmx.h)
__device__ __forceinline__ uint32_t bot_hash(uint32_t key, uint32_t ticks, int agent, uint32_t salt)
{
    uint32_t x = key ^ (ticks * 0x85EBCA77u) ^ ((uint32_t)agent * 0xC2B2AE3Du) ^ salt;
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}

// ---------------------------------------------------------------------------------------------------------------
// Belief sets of the hidden enemies (include/pmx.h, "Belief sets"): per learner slot and enemy the set of cells the enemy can be
// on, one row word per board row -- the bit-board form of the tick.  One wavefront per ENV, four envs per block; lane = enemy *
// 32 + row, so a lane owns one row word of one enemy's set and both enemies advance side by side.  The agent words of the two
// learners' snapshots are read once (lanes 0-3 and 4-7) and broadcast as scalars; the vertical neighbours of the motion step come
// from width-32 shuffles (row 0 takes 0 from below, row 31 0 from above; rows >= H hold 0); the sight discs and the sonar annulus
// of a row are spans of bits around the observer's column whose half-width follows from |y - oy|, so no cell is visited.  The wave
// reads the previous call's slot-1 sets (the 256 bytes of the env's 512-byte block that the rule uses) and writes both halves of
// the block, 256 contiguous bytes per instruction; no LDS.
// ---------------------------------------------------------------------------------------------------------------
#define PMX_SALT_SONAR 0x534F4E41u      // the sonar's noise draw (include/pmx.h)

// bits ox - w .. ox + w of a row, clipped to the word; none when w < 0
__device__ __forceinline__ uint32_t belief_span(int ox, int w)
{
    if (w < 0) return 0u;
    const int lo = ox - w > 0 ? ox - w : 0, hi = ox + w < 31 ? ox + w : 31;
    return (0xFFFFFFFFu >> (31 - hi)) & (0xFFFFFFFFu << lo);
}

__device__ __forceinline__ int belief_manhattan(uint32_t a, uint32_t b)
{
    return abs((int)(a & 0xFF) - (int)(b & 0xFF)) + abs((int)((a >> 8) & 0xFF) - (int)((b >> 8) & 0xFF));
}

// ---------------------------------------------------------------------------------------------------------------
// Belief evidence (include/pmx.h, "Belief evidence"): three public facts the observation leaves on a hidden enemy -- its side, the
// pellet it ate, and that it can only have died next to one of the team's agents -- as the EVIDENCE form of the two update bodies
// below.  Off (the parents' kernels) none of this is compiled.  On, a lane also takes row y of the food in both slots'
// snapshots and, lanes 0-35, its word of the env's evidence row (one coalesced load; the food rows reach both halves by a shuffle
// from lane y, the three scalars by readlane).  "Exactly one pellet left" and "the set touches K" are wave-uniform decisions on a
// 64-bit ballot, half 0 of it for the pellet, the lane's own half for K; the pellet's cell is a readlane of the one non-zero row; K
// is four spans of half-width 1 - |y - qy|.  No LDS, no atomics; the new row is one vector store by lanes 0-35, each the lane that
// loaded the old word (same lane, same address, in order).
// ---------------------------------------------------------------------------------------------------------------
#define PMX_EVIDENCE_SIDE 1             // the rule bits and the evidence row's width (include/pmx.h)
#define PMX_EVIDENCE_FOOD 2
#define PMX_EVIDENCE_CONTACT 4
#define PMX_EVIDENCE_WORDS 36

// the second argument of the two update kernels: the evidence block in the EVIDENCE form, nothing otherwise
template <bool EVIDENCE> struct BeliefEvidenceArg {};
template <> struct BeliefEvidenceArg<true> : PmxBeliefEvidenceParams {};

struct BeliefEvidence {
    uint32_t F0, F1, Fe;        // row y of the food in slot 0's and slot 1's snapshot and in the evidence row
    uint32_t qf, qs;            // the team's two cells in the previous snapshot of the slot at hand (x | y << 8)
    uint32_t sf, ss;            // the start cells of `first` and `second`
    uint32_t lo, hi, mine;      // columns x < half, x >= half, and the half the team defends
    int32_t half, rules;
    bool valid;                 // the evidence row held a snapshot
};

// step 5: the evidence row from slot 1's snapshot `snap1` (this env's word 0), valid = 1; reset rows too
__device__ __forceinline__ void belief_evidence_store(uint32_t *Ev, const uint32_t *snap1, int lane, int H, size_t N, int first, int second)
{
    uint32_t v = lane == 34 ? 1u : 0u;
    if (lane < H) v = snap1[(size_t)lane * N];
    if (lane == 32 || lane == 33) v = snap1[(size_t)PMX_W_AGENT_A(H, lane == 32 ? first : second) * N] & 0xFFFFu;
    if (lane < PMX_EVIDENCE_WORDS) Ev[lane] = v;
}

__device__ __forceinline__ BeliefEvidence belief_evidence_load(const PmxBeliefEvidenceParams &e, const PmxLayoutDev *L, const uint32_t *Ev,
                                                              const uint32_t *snap0, const uint32_t *snap1, int lane, int H, size_t N,
                                                              int first, int second)
{
    BeliefEvidence v;
    const int y = lane & 31;
    v.F0 = y < H ? snap0[(size_t)y * N] : 0u;
    v.F1 = y < H ? snap1[(size_t)y * N] : 0u;
    const uint32_t ew = lane < PMX_EVIDENCE_WORDS ? Ev[lane] : 0u;
    v.Fe = __shfl(ew, y);
    v.qf = (uint32_t)__builtin_amdgcn_readlane((int)ew, 32);
    v.qs = (uint32_t)__builtin_amdgcn_readlane((int)ew, 33);
    v.valid = __builtin_amdgcn_readlane((int)ew, 34) != 0;
    v.sf = (uint32_t)(L->startx[first] | (L->starty[first] << 8));
    v.ss = (uint32_t)(L->startx[second] | (L->starty[second] << 8));
    v.lo = L->lo_mask, v.hi = L->hi_mask, v.mine = first ? v.hi : v.lo;
    v.half = L->half;
    v.rules = e.rules;
    return v;
}

// the cells of row y within Manhattan distance 1 of q
__device__ __forceinline__ uint32_t belief_near(uint32_t q, int y)
{
    return belief_span((int)(q & 0xFF), 1 - abs(y - (int)((q >> 8) & 0xFF)));
}

// steps 2a and 3 of slot j on the lane's row S of enemy k's set, after the dilation.  Every lane of the wave calls it
__device__ __forceinline__ uint32_t belief_evidence_food_respawn(const BeliefEvidence &v, int j, int k, int y, bool moved, uint32_t S, uint32_t start_bit)
{
    const bool has_prev = j ? true : v.valid;                   // slot 1's previous snapshot is slot 0's
    if ((v.rules & PMX_EVIDENCE_FOOD) && has_prev) {            // 2a: the one pellet that left the defended half pins the mover
        const uint32_t E = (j ? v.F0 : v.Fe) & ~(j ? v.F1 : v.F0) & v.mine;
        const uint32_t rows = (uint32_t)__ballot(E != 0u);      // half 0: bit y = row y of E is not empty
        const int yc = rows ? __builtin_ctz(rows) : 0;
        const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)E, yc);
        if ((rows & (rows - 1u)) == 0u && w != 0u && (w & (w - 1u)) == 0u) {
            const uint32_t c = (uint32_t)__builtin_ctz(w) | ((uint32_t)yc << 8);
            // not if the learner can have eaten it: one step from where it was, or from its start if it was killed in between
            if (belief_manhattan(c, j ? v.qs : v.qf) > 1 && belief_manhattan(c, j ? v.ss : v.sf) > 1 && moved) S &= E;
        }
    }
    if ((v.rules & PMX_EVIDENCE_CONTACT) && has_prev) {         // 3: a death is a collision with one of the team's agents
        const uint32_t K = belief_near(v.qf, y) | belief_near(v.qs, y) | belief_near(v.sf, y) | belief_near(v.ss, y);
        const uint64_t touch = __ballot((S & K) != 0u);
        return (uint32_t)(touch >> (32 * k)) != 0u ? S | start_bit : S;
    }
    return S | start_bit;
}

template <bool INIT, bool EVIDENCE = false>
__global__ __launch_bounds__(PMX_BLOCK) void pmx_belief_kernel(PmxBeliefParams p, BeliefEvidenceArg<EVIDENCE> e)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int k = lane >> 5, y = lane & 31;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= p.count) return;
    const long env = row + p.first;
    const int W = p.lay_W, H = p.lay_H;
    const size_t N = (size_t)p.N;
    const PmxLayoutDev *L = p.lay + (p.layout_idx ? p.layout_idx[env] : 0);
    uint32_t *B = p.belief + (size_t)row * 128 + lane;          // [slot][enemy][row]: word slot * 64 + lane
    const uint32_t open = y < H ? ~L->walls[y] & (W == 32 ? 0xFFFFFFFFu : (1u << W) - 1u) : 0u;
    if constexpr (INIT) {
        // kind 1: every open cell (the state was set from outside, or the colour changed).  kind 0: the start cells of agents 2 k
        // and 2 k + 1, enemy k of a blue and of a red team -- the call takes no colour
        const uint32_t s = p.kind != 0 ? open : ((y == L->starty[2 * k] ? 1u << L->startx[2 * k] : 0u) |
                                                 (y == L->starty[2 * k + 1] ? 1u << L->startx[2 * k + 1] : 0u));
        B[0] = s;
        B[64] = s;
        return;
    }
    const int red_v = p.team_red ? __builtin_amdgcn_readfirstlane((int)p.team_red[env]) : p.red;
    const int first = red_v ? 0 : 1, second = first + 2;
    const int e_k = (1 - first) + 2 * k;
    const uint32_t start_bit = y == L->starty[e_k] ? 1u << L->startx[e_k] : 0u;
    if (p.reset && __builtin_amdgcn_readfirstlane((int)p.reset[env]) != 0) {
        B[0] = start_bit;
        B[64] = start_bit;
        if (p.sonar && y < 2) p.sonar[(size_t)row * 4 + y * 2 + k] = 0;       // no reading is taken at a reset
        if constexpr (EVIDENCE) belief_evidence_store(e.evidence + (size_t)row * PMX_EVIDENCE_WORDS, p.snap[second] + env, lane, H, N, first, second);
        return;
    }
    if constexpr (!INIT) {
        uint32_t S = B[64];                                     // the previous call's slot 1
        uint32_t aw = 0;                                        // lanes 0-3: slot 0's snapshot, lanes 4-7: slot 1's
        if (lane < 8) aw = (p.snap[lane < 4 ? first : second] + env)[(size_t)PMX_W_AGENT_A(H, lane & 3) * N] & 0xFFFFu;
        const uint32_t ticks = p.state[(size_t)PMX_W_TICKS(H) * N + env];
        const uint32_t key = p.seed ^ ((uint32_t)env * 0x9E3779B1u);
        [[maybe_unused]] BeliefEvidence v;
        if constexpr (EVIDENCE) v = belief_evidence_load(e, L, e.evidence + (size_t)row * PMX_EVIDENCE_WORDS, p.snap[first] + env, p.snap[second] + env, lane, H, N, first, second);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int a_j = first + 2 * j;
            // the team's two agents and the two enemies in slot j's snapshot (wave-uniform)
            const uint32_t p0 = (uint32_t)__builtin_amdgcn_readlane((int)aw, 4 * j + 0), p1 = (uint32_t)__builtin_amdgcn_readlane((int)aw, 4 * j + 1);
            const uint32_t p2 = (uint32_t)__builtin_amdgcn_readlane((int)aw, 4 * j + 2), p3 = (uint32_t)__builtin_amdgcn_readlane((int)aw, 4 * j + 3);
            const uint32_t pf = first ? p1 : p0, ps = first ? p3 : p2;
            const uint32_t pa = j ? ps : pf, pe = first ? (k ? p2 : p0) : (k ? p3 : p1);
            // motion: the enemy whose sub-step lies between the two snapshots (Stop included).  Every lane runs the shuffles
            const uint32_t up = __shfl_down(S, 1, 32), dn = __shfl_up(S, 1, 32);
            if (e_k == ((a_j + 3) & 3)) S = (S | (S << 1) | (S >> 1) | (y < 31 ? up : 0u) | (y > 0 ? dn : 0u)) & open;
            if constexpr (EVIDENCE) S = belief_evidence_food_respawn(v, j, k, y, e_k == ((a_j + 3) & 3), S, start_bit);
            else S |= start_bit;                                // every death returns an agent to its start
            const uint32_t h = bot_hash(key, ticks, 4 * a_j + e_k, PMX_SALT_SONAR);
            const int r = belief_manhattan(pa, pe) + (int)(((uint64_t)h * 13u) >> 32) - 6;
            const int df = belief_manhattan(pe, pf), ds = belief_manhattan(pe, ps);
            if ((df < ds ? df : ds) <= p.sight) {
                S = y == (int)(pe >> 8) ? 1u << (pe & 0xFF) : 0u;
            } else {
                const int dyf = abs(y - (int)(pf >> 8)), dys = abs(y - (int)(ps >> 8)), dya = abs(y - (int)(pa >> 8));
                S &= ~(belief_span((int)(pf & 0xFF), p.sight - dyf) | belief_span((int)(ps & 0xFF), p.sight - dys));
                S &= belief_span((int)(pa & 0xFF), r + 6 - dya) & ~belief_span((int)(pa & 0xFF), r - 7 - dya);
                // 4: the isPacman flag a hidden enemy keeps, taken from its position
                if constexpr (EVIDENCE) if (v.rules & PMX_EVIDENCE_SIDE) S &= (int)(pe & 0xFF) < v.half ? v.lo : v.hi;
            }
            B[64 * j] = S;
            if (p.sonar && y == 0) p.sonar[(size_t)row * 4 + j * 2 + k] = (int8_t)r;
            if constexpr (EVIDENCE) v.qf = pf, v.qs = ps;
        }
        if constexpr (EVIDENCE) belief_evidence_store(e.evidence + (size_t)row * PMX_EVIDENCE_WORDS, p.snap[second] + env, lane, H, N, first, second);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Belief weights (include/pmx.h, "Belief weights"): the exact Bayes filter that refines the sets -- a uint16 weight per learner
// slot, enemy and cell, and the uint8 levels the weighted emission shows.  A kernel of its own beside pmx_belief_kernel, whose code
// stays what it is; the two share belief_span, belief_manhattan, bot_hash and the snapshot / readlane set-up, and this one runs the
// set rule word for word, so belief and sonar come out as pmx_belief_update leaves them.
// One wavefront per env, four per block.  The SET part keeps the set kernel's shape (lane = enemy * 32 + row, one row word per
// lane).  The WEIGHT part deals the cells of an enemy's board to the 32 lanes of its half, cell c = c0 + (lane & 31): global loads
// and stores of a half are 64 / 32 consecutive bytes and an 18 x 11 board takes 7 rounds instead of 20 walks along a row with two
// thirds of the lanes idle.  y = c / W is a multiplication by ceil(65536 / W), exact for c < 1055 and W <= 32.  A cell's open bit,
// its four neighbours' and its bit of S' come from width-32 shuffles of the row words the set part holds, so no distance is
// evaluated per cell.  (Keeping column, row and open bits per cell as a 16-bit word in LDS instead of recomputing them in every
// round measured no faster: 57.4 against 54.2 us at 16 384 smallCapture envs.)  Per slot, three rounds over the cells, all lanes of the wave in step (exactly one of the two enemies moved,
// so nothing is gained by branching on it):
//   A  a[c] = moved ? (open ? (q[c] * R[deg(c)]) >> 16 : 0) : q[c]  into LDS (uint16 [enemy][1024], 4 KB per wave).  q is read
//      from global: the previous call's slot 1, then the slot 0 this lane itself has just stored (same lane, same address);
//   B  t[c] = moved ? a[c] + the a of c's open neighbours (0 on walls) : a[c];  T = sum t,  m0 = max over S' minus the start cell
//      of max(t, 1),  t at the start cell: three reductions within the 32-lane half.  Then add = 1 + (T >> RESPAWN_SHIFT),
//      m = max(m0, t[start] + add if the start cell is in S'), b = 32 - clz(m);
//   C  t again (five LDS reads are cheaper than keeping 19-bit values), u, q' by the shift; q' to global, the level to the
//      other half by one xor-32 shuffle, the larger one stored by half 0.
// LDS operations of one wavefront execute in order; the wave fences between the rounds keep the compiler from moving them.
// No atomics, no floating point, vector stores only.
// ---------------------------------------------------------------------------------------------------------------
#define PMX_BELIEF_RESPAWN_SHIFT 7      // include/pmx.h

struct BeliefCell { int x, y; uint32_t me, l, r, u, d; };    // a cell's column and row, its own open bit and its neighbours'

__device__ __forceinline__ BeliefCell belief_cell(int c, int W, int inv, uint32_t open)
{
    BeliefCell g;
    const int yr = (c * inv) >> 16;
    g.x = c - yr * W;                   // 0 .. W - 1 for every c < 1055
    g.y = yr & 31;                      // (lanes past the board compute a row of no meaning; their results are not used)
    const uint32_t om = __shfl(open, g.y, 32), ou = __shfl(open, (g.y + 31) & 31, 32), od = __shfl(open, (g.y + 1) & 31, 32);
    g.me = (om >> g.x) & 1u;
    g.l = g.x > 0 ? (om >> (g.x - 1)) & 1u : 0u;
    g.r = g.x < 31 ? (om >> (g.x + 1)) & 1u : 0u;
    g.u = g.y > 0 ? (ou >> g.x) & 1u : 0u;
    g.d = g.y < 31 ? (od >> g.x) & 1u : 0u;
    return g;
}

__device__ __forceinline__ uint32_t belief_half_sum(uint32_t v)
{
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 32);
    return v;
}

__device__ __forceinline__ uint32_t belief_half_max(uint32_t v)
{
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
        const uint32_t w = __shfl_xor(v, o, 32);
        v = w > v ? w : v;
    }
    return v;
}

template <bool INIT, bool EVIDENCE = false>
__global__ __launch_bounds__(PMX_BLOCK) void pmx_belief_weights_kernel(PmxBeliefWeightsParams pw, BeliefEvidenceArg<EVIDENCE> e)
{
    __shared__ uint16_t contrib[4][2][1024];                    // [wave][enemy][cell]: round A's a[c]
    const PmxBeliefParams &p = pw.b;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int k = lane >> 5, y = lane & 31;
    const long row = (long)blockIdx.x * 4 + wave;
    if (row >= p.count) return;
    const long env = row + p.first;
    const int W = p.lay_W, H = p.lay_H, HW = H * W;
    const int inv = (65536 + W - 1) / W;
    const size_t N = (size_t)p.N;
    const PmxLayoutDev *L = p.lay + (p.layout_idx ? p.layout_idx[env] : 0);
    uint32_t *B = p.belief + (size_t)row * 128 + lane;          // [slot][enemy][row]: word slot * 64 + lane
    uint16_t *Wt = pw.weights + ((size_t)row * 4 + k) * HW;     // [slot][enemy][cell]: slot j at + j * 2 * HW
    uint8_t *Lv = pw.levels + (size_t)row * 2 * HW;             // [slot][cell]
    const uint32_t open = y < H ? ~L->walls[y] & (W == 32 ? 0xFFFFFFFFu : (1u << W) - 1u) : 0u;

    // both slots of both enemies: 65535 on the cells of the set S (a row word per lane), 0 elsewhere, and the levels to match
    auto store_set = [&](uint32_t S) {
        for (int c0 = 0; c0 < HW; c0 += 32) {
            const int c = c0 + y;
            const int yr = (c * inv) >> 16, xc = c - yr * W;
            const uint32_t on = c < HW ? (__shfl(S, yr & 31, 32) >> xc) & 1u : 0u;
            const uint32_t other = __shfl_xor(on, 32);
            if (c < HW) {
                Wt[c] = on ? 65535 : 0;
                Wt[2 * HW + c] = on ? 65535 : 0;
                if (k == 0) {
                    Lv[c] = (on | other) ? 16 : 0;
                    Lv[HW + c] = (on | other) ? 16 : 0;
                }
            }
        }
    };

    if constexpr (INIT) {
        const uint32_t s = p.kind != 0 ? open : ((y == L->starty[2 * k] ? 1u << L->startx[2 * k] : 0u) |
                                                 (y == L->starty[2 * k + 1] ? 1u << L->startx[2 * k + 1] : 0u));
        B[0] = s;
        B[64] = s;
        store_set(s);
        return;
    }
    const int red_v = p.team_red ? __builtin_amdgcn_readfirstlane((int)p.team_red[env]) : p.red;
    const int first = red_v ? 0 : 1, second = first + 2;
    const int e_k = (1 - first) + 2 * k;
    const uint32_t start_bit = y == L->starty[e_k] ? 1u << L->startx[e_k] : 0u;
    const int start_c = L->starty[e_k] * W + L->startx[e_k];
    if (p.reset && __builtin_amdgcn_readfirstlane((int)p.reset[env]) != 0) {
        B[0] = start_bit;
        B[64] = start_bit;
        if (p.sonar && y < 2) p.sonar[(size_t)row * 4 + y * 2 + k] = 0;
        store_set(start_bit);
        if constexpr (EVIDENCE) belief_evidence_store(e.evidence + (size_t)row * PMX_EVIDENCE_WORDS, p.snap[second] + env, lane, H, N, first, second);
        return;
    }
    if constexpr (!INIT) {
        uint16_t *A = contrib[wave][k];
        uint32_t S = B[64];                                     // the previous call's slot 1
        uint32_t aw = 0;                                        // lanes 0-3: slot 0's snapshot, lanes 4-7: slot 1's
        if (lane < 8) aw = (p.snap[lane < 4 ? first : second] + env)[(size_t)PMX_W_AGENT_A(H, lane & 3) * N] & 0xFFFFu;
        const uint32_t ticks = p.state[(size_t)PMX_W_TICKS(H) * N + env];
        const uint32_t key = p.seed ^ ((uint32_t)env * 0x9E3779B1u);
        [[maybe_unused]] BeliefEvidence v;
        if constexpr (EVIDENCE) v = belief_evidence_load(e, L, e.evidence + (size_t)row * PMX_EVIDENCE_WORDS, p.snap[first] + env, p.snap[second] + env, lane, H, N, first, second);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            // ---- the set rule, as in pmx_belief_kernel ----
            const int a_j = first + 2 * j;
            const uint32_t p0 = (uint32_t)__builtin_amdgcn_readlane((int)aw, 4 * j + 0), p1 = (uint32_t)__builtin_amdgcn_readlane((int)aw, 4 * j + 1);
            const uint32_t p2 = (uint32_t)__builtin_amdgcn_readlane((int)aw, 4 * j + 2), p3 = (uint32_t)__builtin_amdgcn_readlane((int)aw, 4 * j + 3);
            const uint32_t pf = first ? p1 : p0, ps = first ? p3 : p2;
            const uint32_t pa = j ? ps : pf, pe = first ? (k ? p2 : p0) : (k ? p3 : p1);
            const bool moved = e_k == ((a_j + 3) & 3);
            const uint32_t up = __shfl_down(S, 1, 32), dn = __shfl_up(S, 1, 32);
            if (moved) S = (S | (S << 1) | (S >> 1) | (y < 31 ? up : 0u) | (y > 0 ? dn : 0u)) & open;
            if constexpr (EVIDENCE) S = belief_evidence_food_respawn(v, j, k, y, moved, S, start_bit);
            else S |= start_bit;
            const uint32_t h = bot_hash(key, ticks, 4 * a_j + e_k, PMX_SALT_SONAR);
            const int r = belief_manhattan(pa, pe) + (int)(((uint64_t)h * 13u) >> 32) - 6;
            const int df = belief_manhattan(pe, pf), ds = belief_manhattan(pe, ps);
            const bool seen = (df < ds ? df : ds) <= p.sight;
            if (seen) {
                S = y == (int)(pe >> 8) ? 1u << (pe & 0xFF) : 0u;
            } else {
                const int dyf = abs(y - (int)(pf >> 8)), dys = abs(y - (int)(ps >> 8)), dya = abs(y - (int)(pa >> 8));
                S &= ~(belief_span((int)(pf & 0xFF), p.sight - dyf) | belief_span((int)(ps & 0xFF), p.sight - dys));
                S &= belief_span((int)(pa & 0xFF), r + 6 - dya) & ~belief_span((int)(pa & 0xFF), r - 7 - dya);
                if constexpr (EVIDENCE) if (v.rules & PMX_EVIDENCE_SIDE) S &= (int)(pe & 0xFF) < v.half ? v.lo : v.hi;
            }
            B[64 * j] = S;
            if (p.sonar && y == 0) p.sonar[(size_t)row * 4 + j * 2 + k] = (int8_t)r;
            if constexpr (EVIDENCE) v.qf = pf, v.qs = ps;

            // ---- the weights of slot j: q = slot 1 of the previous call (j == 0) or the slot 0 just stored (j == 1) ----
            const uint16_t *Qg = Wt + (1 - j) * 2 * HW;
            uint16_t *Og = Wt + j * 2 * HW;
            const int pe_c = (int)(pe >> 8) * W + (int)(pe & 0xFF);
            // t[c] of the motion step from round A's a[]; called with c < HW only
            auto t_of = [&](int c, const BeliefCell &g) -> uint32_t {
                uint32_t t = A[c];
                if (moved) {
                    if (g.l) t += A[c - 1];
                    if (g.r) t += A[c + 1];
                    if (g.u) t += A[c - W];
                    if (g.d) t += A[c + W];
                    if (!g.me) t = 0;
                }
                return t;
            };
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // slot 0's round C has read a[] for the last time
            __builtin_amdgcn_wave_barrier();
            for (int c0 = 0; c0 < HW; c0 += 32) {                       // round A
                const int c = c0 + y;
                const BeliefCell g = belief_cell(c, W, inv, open);
                if (c < HW) {
                    const uint32_t q = Qg[c];
                    const int deg = 1 + (int)(g.l + g.r + g.u + g.d);
                    const uint32_t R = deg == 1 ? 65536u : (deg == 2 ? 32768u : (deg == 3 ? 21845u : (deg == 4 ? 16384u : 13107u)));
                    A[c] = (uint16_t)(moved ? (g.me ? (q * R) >> 16 : 0u) : q);     // q <= 65535, R <= 65536: the product is below 2^32
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            uint32_t T = 0, m0 = 0, t_start = 0;
            for (int c0 = 0; c0 < HW; c0 += 32) {                       // round B
                const int c = c0 + y;
                const BeliefCell g = belief_cell(c, W, inv, open);
                const uint32_t in_set = (__shfl(S, g.y, 32) >> g.x) & 1u;
                if (c < HW) {
                    const uint32_t t = t_of(c, g);                       // <= 5 * 65535
                    T += t;                                              // <= 1024 * 5 * 65535 < 2^32
                    if (c == start_c) t_start = t;
                    else if (in_set) m0 = m0 > t ? m0 : (t > 1u ? t : 1u);
                }
            }
            T = belief_half_sum(T);
            m0 = belief_half_max(m0);
            t_start = belief_half_max(t_start);
            const uint32_t start_in = belief_half_max((S & start_bit) != 0u ? 1u : 0u);
            const uint32_t add = 1u + (T >> PMX_BELIEF_RESPAWN_SHIFT);
            const uint32_t u_start = start_in ? t_start + add : 0u;     // < 2^22
            const uint32_t m = m0 > u_start ? m0 : u_start;
            const int b = 32 - __clz((int)m);                           // 0 for an empty set
            for (int c0 = 0; c0 < HW; c0 += 32) {                       // round C
                const int c = c0 + y;
                const BeliefCell g = belief_cell(c, W, inv, open);
                const uint32_t in_set = (__shfl(S, g.y, 32) >> g.x) & 1u;
                uint32_t lev = 0;
                if (c < HW) {
                    uint32_t q = 0;
                    if (seen) {
                        q = c == pe_c ? 65535u : 0u;
                    } else if (in_set) {
                        const uint32_t t = t_of(c, g);
                        const uint32_t u = c == start_c ? t + add : (t > 1u ? t : 1u);
                        if (b > 16) {
                            q = u >> (b - 16);
                            q = q > 1u ? q : 1u;
                        } else {
                            q = u << (16 - b);
                        }
                    }
                    Og[c] = (uint16_t)q;
                    lev = q ? 1u + (q >> 12) : 0u;
                }
                const uint32_t lev_o = __shfl_xor(lev, 32);
                if (c < HW && k == 0) Lv[j * HW + c] = (uint8_t)(lev > lev_o ? lev : lev_o);
            }
        }
        if constexpr (EVIDENCE) belief_evidence_store(e.evidence + (size_t)row * PMX_EVIDENCE_WORDS, p.snap[second] + env, lane, H, N, first, second);
    }
}

