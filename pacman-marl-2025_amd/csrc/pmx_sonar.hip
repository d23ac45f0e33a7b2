// pmx_sonar.hip -- pmx_agent_distances (include/pmx.h, "Sight rule on the four-agent planes"): the contest's getAgentDistances()
// for every env, the four noisy distances an agent gets beside its observation.  A code object of its own, so that the kernels of the
// other files stay the instructions they were.  gfx950 only.
#include <hip/hip_ext.h>

#include "pmx_belief.h"                 // bot_hash, belief_manhattan, PMX_SALT_SONAR: the draw pmx_belief_update makes

// One lane per ENV, one wavefront per block (as the rule kernels: N / 64 blocks spread over the CUs).  ALL: a lane loads the four
// agent-A words of each of the four sources (agent a's snapshot after a pmx_step, the state otherwise) and the tick word -- 17
// coalesced dword streams in the state's own word-major order, all issued before the first is used, so the kernel is one HBM round
// trip deep -- makes the 16 draws in registers and stores its 16 readings r[a][i] with one 16-byte store.  Single agent: the four
// words of the state, four draws, one 4-byte store.  No LDS, no atomics.
struct PmxSonarParams {
    const uint32_t *snap[4];     // per source agent a: the words its readings are taken from (ALL); [0] = the state (single agent)
    const uint32_t *state;       // the env's state words: the tick counter keys the draw
    int8_t *dist;                // [N][4][4] (ALL) or [N][4]
    int32_t N, lay_H, agent;     // agent: the observer of the single-agent form
    uint32_t seed;
};

__device__ __forceinline__ uint32_t sonar_reading(uint32_t key, uint32_t ticks, int a, int i, uint32_t pa, uint32_t pi)
{
    const uint32_t h = bot_hash(key, ticks, 4 * a + i, PMX_SALT_SONAR);
    return (uint32_t)(belief_manhattan(pa, pi) + (int)(((uint64_t)h * 13u) >> 32) - 6) & 0xFFu;      // the int8 reading as a byte
}

template <bool ALL>
__global__ __launch_bounds__(PMX_RULE_BLOCK) void pmx_agent_distances_kernel(PmxSonarParams p)
{
    const long env = (long)blockIdx.x * PMX_RULE_BLOCK + threadIdx.x;
    if (env >= p.N) return;
    const size_t N = (size_t)p.N;
    const int H = p.lay_H;
    const uint32_t ticks = p.state[(size_t)PMX_W_TICKS(H) * N + env];
    const uint32_t key = p.seed ^ ((uint32_t)env * 0x9E3779B1u);
    if constexpr (ALL) {
        uint32_t w[4][4];                                             // every load of the lane before the first use
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int i = 0; i < 4; ++i) w[a][i] = p.snap[a][(size_t)PMX_W_AGENT_A(H, i) * N + env];
        uint32_t r[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            r[a] = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) r[a] |= sonar_reading(key, ticks, a, i, w[a][a], w[a][i]) << (8 * i);
        }
        reinterpret_cast<uint4 *>(p.dist)[env] = make_uint4(r[0], r[1], r[2], r[3]);
    } else {
        const int a = p.agent;
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = p.snap[0][(size_t)PMX_W_AGENT_A(H, i) * N + env];
        const uint32_t pa = a == 0 ? w[0] : (a == 1 ? w[1] : (a == 2 ? w[2] : w[3]));     // selects, never an index into registers
        uint32_t r = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) r |= sonar_reading(key, ticks, a, i, pa, w[i]) << (8 * i);
        reinterpret_cast<uint32_t *>(p.dist)[env] = r;
    }
}

// agent -1: all 16 readings from snap[0..3]; agent 0 .. 3: that agent's four readings from `state`.  ev0 / ev1 as in pmx_launch_belief
extern "C" hipError_t pmx_launch_agent_distances(const uint32_t *const *snap, const uint32_t *state, int8_t *dist, int N, int H, int agent,
                                                 uint32_t seed, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
{
    PmxSonarParams p;
    for (int a = 0; a < 4; ++a) p.snap[a] = agent < 0 ? snap[a] : state;
    p.state = state;
    p.dist = dist;
    p.N = N, p.lay_H = H, p.agent = agent;
    p.seed = seed;
    const unsigned blocks = (unsigned)(((long)N + PMX_RULE_BLOCK - 1) / PMX_RULE_BLOCK);
#define PMX_SONAR(ALL)                                                                                                              \
    do {                                                                                                                            \
        if (ev0) hipExtLaunchKernelGGL((pmx_agent_distances_kernel<ALL>), dim3(blocks), dim3(PMX_RULE_BLOCK), 0, st, ev0, ev1, 0, p); \
        else hipLaunchKernelGGL((pmx_agent_distances_kernel<ALL>), dim3(blocks), dim3(PMX_RULE_BLOCK), 0, st, p);                    \
    } while (0)
    if (agent < 0) PMX_SONAR(true); else PMX_SONAR(false);
#undef PMX_SONAR
    return hipGetLastError();
}
