// pmx_stats.hip -- episode statistics (include/pmx.h, "Episode statistics"): an exact per-episode event record for every env, counted
// from the sub-step snapshots a tick leaves.  A code object of its own, so that the kernels of the other files stay the instructions
// they were.  gfx950 only.
#include <hip/hip_ext.h>

#include "pmx_device.h"

// One lane per ENV, one wavefront per block (as the rule kernels: count / 64 blocks spread over the CUs).  A lane loads its row of
// the record (43 words used) and the 10 agent / capsule words of the three snapshots and the state (+ the score word): every one
// a coalesced dword stream in the state's own word-major order, all issued before the first is used, so the kernel is one HBM round
// trip deep.  The four transitions are then register arithmetic.  No LDS, no atomics; the row goes back with plain dword stores,
// each by the lane that loaded the word.  A finished row (DONE != 0) stores nothing.
#define PMX_STATS_WORDS 48              // include/pmx.h
#define PMX_STATS_W_TICKS 32
#define PMX_STATS_W_SCORE 33
#define PMX_STATS_W_DONE 34
#define PMX_STATS_W_STATE 36            // 36..39 agent words A, 40..43 agent words B, 44..45 capsule words
enum { ST_EATEN, ST_RETURNED, ST_LOST, ST_DEATHS, ST_KILLS, ST_CAPSULES, ST_PACMAN_STEPS, ST_STOPS };

struct StatsState {                     // the ten words of a snapshot the rules below read
    uint32_t a[4], b[4], cap[2];
};

__device__ __forceinline__ StatsState stats_load_snap(const uint32_t *S, int H, size_t N)      // S: word 0 of this lane's env
{
    StatsState s;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s.a[i] = S[(size_t)PMX_W_AGENT_A(H, i) * N];
        s.b[i] = S[(size_t)PMX_W_AGENT_B(H, i) * N];
    }
    s.cap[0] = S[(size_t)PMX_W_CAPS(H, 0) * N];
    s.cap[1] = S[(size_t)PMX_W_CAPS(H, 1) * N];
    return s;
}

__device__ __forceinline__ int stats_caps(const StatsState &s)          // occupied capsule slots (0xFFFF = empty)
{
    return ((s.cap[0] & 0xFFFFu) != 0xFFFFu) + ((s.cap[0] >> 16) != 0xFFFFu) + ((s.cap[1] & 0xFFFFu) != 0xFFFFu) + ((s.cap[1] >> 16) != 0xFFFFu);
}

__device__ __forceinline__ int st_x(uint32_t a) { return (int)(a & 0xFF); }
__device__ __forceinline__ int st_y(uint32_t a) { return (int)((a >> 8) & 0xFF); }
__device__ __forceinline__ int st_pac(uint32_t a) { return (int)((a >> 24) & 1); }
__device__ __forceinline__ int st_scared(uint32_t b) { return (int)(b & 0xFF); }
__device__ __forceinline__ int st_carry(uint32_t b) { return (int)((b >> 8) & 0xFFF); }
__device__ __forceinline__ int st_ret(uint32_t b) { return (int)((b >> 20) & 0xFFF); }

// the transition X -> Y made by mover M (the table of include/pmx.h)
template <int M>
__device__ __forceinline__ void stats_transition(const StatsState &X, const StatsState &Y, int32_t (&c)[4][8])
{
    int kills = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i == M) continue;
        const bool died = (Y.a[i] & 0xFFFFu) != (X.a[i] & 0xFFFFu) || (st_scared(X.b[i]) > 0 && st_scared(Y.b[i]) == 0) ||
                          st_carry(Y.b[i]) < st_carry(X.b[i]);
        if (died) {
            c[i][ST_DEATHS] += 1;
            c[i][ST_LOST] += st_carry(X.b[i]);
            kills += 1;
        }
    }
    const int dist = abs(st_x(Y.a[M]) - st_x(X.a[M])) + abs(st_y(Y.a[M]) - st_y(X.a[M]));
    const int cx = st_carry(X.b[M]), cy = st_carry(Y.b[M]);
    const bool died = dist > 1 || (cy < cx && st_ret(Y.b[M]) == st_ret(X.b[M])) || (st_scared(X.b[M]) >= 2 && st_scared(Y.b[M]) == 0);
    if (died) {
        c[M][ST_DEATHS] += 1;
        c[M][ST_LOST] += cx;
    }
    c[M][ST_KILLS] += kills;
    c[M][ST_EATEN] += cy > cx ? cy - cx : 0;
    c[M][ST_RETURNED] += st_ret(Y.b[M]) - st_ret(X.b[M]);
    c[M][ST_CAPSULES] += stats_caps(X) - stats_caps(Y);
    c[M][ST_PACMAN_STEPS] += st_pac(Y.a[M]);
    c[M][ST_STOPS] += (!died && dist == 0) ? 1 : 0;
}

struct PmxStatsParams {
    const uint32_t *snap[4];     // the states after sub-steps 0, 1, 2 and the current state
    const uint8_t *done;         // [N] or NULL
    int32_t *stats;              // [PMX_STATS_WORDS][count]
    int32_t N, first, count, lay_H;
};

__device__ __forceinline__ void stats_store_state(int32_t *R, size_t C, const StatsState &s, int32_t score)
{
    R[(size_t)PMX_STATS_W_SCORE * C] = score;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        R[(size_t)(PMX_STATS_W_STATE + i) * C] = (int32_t)s.a[i];
        R[(size_t)(PMX_STATS_W_STATE + 4 + i) * C] = (int32_t)s.b[i];
    }
    R[(size_t)(PMX_STATS_W_STATE + 8) * C] = (int32_t)s.cap[0];
    R[(size_t)(PMX_STATS_W_STATE + 9) * C] = (int32_t)s.cap[1];
}

template <bool INIT>
__global__ __launch_bounds__(PMX_RULE_BLOCK) void pmx_episode_stats_kernel(PmxStatsParams p)
{
    const long row = (long)blockIdx.x * PMX_RULE_BLOCK + threadIdx.x;
    if (row >= p.count) return;
    const size_t env = (size_t)(row + p.first), N = (size_t)p.N, C = (size_t)p.count;
    const int H = p.lay_H;
    int32_t *R = p.stats + row;                                       // word w of this row: R[w * C]
    const StatsState cur = stats_load_snap(p.snap[3] + env, H, N);
    const int32_t score = (int32_t)p.snap[3][(size_t)PMX_W_SCORE(H) * N + env];
    if constexpr (INIT) {
#pragma unroll
        for (int w = 0; w < PMX_STATS_WORDS; ++w)
            if (w != PMX_STATS_W_SCORE && (w < PMX_STATS_W_STATE || w >= PMX_STATS_W_STATE + 10)) R[(size_t)w * C] = 0;
        stats_store_state(R, C, cur, score);
        return;
    } else {
        // every load of the lane before the first use
        const int32_t was_done = R[(size_t)PMX_STATS_W_DONE * C];
        const uint8_t done = p.done ? p.done[env] : (uint8_t)0;
        const StatsState s0 = stats_load_snap(p.snap[0] + env, H, N);
        const StatsState s1 = stats_load_snap(p.snap[1] + env, H, N);
        const StatsState s2 = stats_load_snap(p.snap[2] + env, H, N);
        StatsState prev;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            prev.a[i] = (uint32_t)R[(size_t)(PMX_STATS_W_STATE + i) * C];
            prev.b[i] = (uint32_t)R[(size_t)(PMX_STATS_W_STATE + 4 + i) * C];
        }
        prev.cap[0] = (uint32_t)R[(size_t)(PMX_STATS_W_STATE + 8) * C];
        prev.cap[1] = (uint32_t)R[(size_t)(PMX_STATS_W_STATE + 9) * C];
        int32_t c[4][8];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < 8; ++k) c[i][k] = R[(size_t)(8 * i + k) * C];
        const int32_t ticks = R[(size_t)PMX_STATS_W_TICKS * C];
        if (was_done != 0) return;                                    // a finished row keeps every word
        stats_transition<0>(prev, s0, c);
        stats_transition<1>(s0, s1, c);
        stats_transition<2>(s1, s2, c);
        stats_transition<3>(s2, cur, c);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < 8; ++k) R[(size_t)(8 * i + k) * C] = c[i][k];
        R[(size_t)PMX_STATS_W_TICKS * C] = ticks + 1;
        R[(size_t)PMX_STATS_W_DONE * C] = done != 0 ? 1 : 0;
        stats_store_state(R, C, cur, score);
    }
}

// count > 0 rows; ev0 / ev1 as in pmx_launch_belief (the update only)
extern "C" hipError_t pmx_launch_episode_stats(const uint32_t *const *snap, const uint8_t *done, int32_t *stats, int N, int first, int count, int H,
                                               int init, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
{
    PmxStatsParams p;
    for (int a = 0; a < 4; ++a) p.snap[a] = snap[a];
    p.done = done;
    p.stats = stats;
    p.N = N, p.first = first, p.count = count, p.lay_H = H;
    const unsigned blocks = (unsigned)(((long)count + PMX_RULE_BLOCK - 1) / PMX_RULE_BLOCK);
    if (init) hipLaunchKernelGGL((pmx_episode_stats_kernel<true>), dim3(blocks), dim3(PMX_RULE_BLOCK), 0, st, p);
    else if (ev0) hipExtLaunchKernelGGL((pmx_episode_stats_kernel<false>), dim3(blocks), dim3(PMX_RULE_BLOCK), 0, st, ev0, ev1, 0, p);
    else hipLaunchKernelGGL((pmx_episode_stats_kernel<false>), dim3(blocks), dim3(PMX_RULE_BLOCK), 0, st, p);
    return hipGetLastError();
}
