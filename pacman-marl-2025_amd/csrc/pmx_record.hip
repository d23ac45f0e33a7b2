// pmx_record.hip -- game records (include/pmx.h, "Game records"): a device log of every sub-step of chosen envs, each frame labelled
// with what happened in it.  A code object of its own, as pmx_stats.hip is, so that the kernels of the other files stay the
// instructions they were.  gfx950 only.
#include <hip/hip_ext.h>

#include "pmx_device.h"

// One lane per ENV, one wavefront per block (as the rule and stats kernels).  head is [PMX_RECORD_HEAD_WORDS][count], frames
// [1 + 4 max_ticks][FW][count], both word-major with the row innermost: every access of a wavefront is one coalesced dword stream.
// The update is two HBM round trips deep, not one: where a row's frames go depends on its LEN word, so the three head words come
// first.  A frozen row (DONE or OVERFLOW) leaves right there, having loaded three words and stored none.  A live row then issues
// every other load -- the previous frame's eleven words, the ten agent / capsule words of the three snapshots and the state, the
// score word, done and the 4 H food rows -- before the first is used; the four EVENT words are register arithmetic.  No LDS, no
// atomics; plain dword stores.
#define PMX_RECORD_HEAD_WORDS 8         // include/pmx.h
enum { RH_LEN, RH_DONE, RH_OVERFLOW, RH_LAYOUT };
#define PMX_RECORD_W_SCORE 10
#define PMX_RECORD_W_EVENT 11
#define PMX_RECORD_W_FOOD 12
#define PMX_RECORD_FW(H) (12 + (H))

// The death rules of include/pmx.h, "Episode statistics", restated from pmx_stats.hip: its kernels do not keep their instructions
// when the rules move into a header both files include (the compiler allocates registers differently), and they must.
// tests/test_game_record_cpu.py and tests/test_gpu_game_record.py hold every death bit written here to the stats model's verdict.
struct RecState {                       // the ten words of a snapshot the rules read
    uint32_t a[4], b[4], cap[2];
};

__device__ __forceinline__ RecState rec_load_snap(const uint32_t *S, int H, size_t N)          // S: word 0 of this lane's env
{
    RecState s;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s.a[i] = S[(size_t)PMX_W_AGENT_A(H, i) * N];
        s.b[i] = S[(size_t)PMX_W_AGENT_B(H, i) * N];
    }
    s.cap[0] = S[(size_t)PMX_W_CAPS(H, 0) * N];
    s.cap[1] = S[(size_t)PMX_W_CAPS(H, 1) * N];
    return s;
}

__device__ __forceinline__ int rec_caps(const RecState &s)              // occupied capsule slots (0xFFFF = empty)
{
    return ((s.cap[0] & 0xFFFFu) != 0xFFFFu) + ((s.cap[0] >> 16) != 0xFFFFu) + ((s.cap[1] & 0xFFFFu) != 0xFFFFu) + ((s.cap[1] >> 16) != 0xFFFFu);
}

__device__ __forceinline__ int rc_x(uint32_t a) { return (int)(a & 0xFF); }
__device__ __forceinline__ int rc_y(uint32_t a) { return (int)((a >> 8) & 0xFF); }
__device__ __forceinline__ int rc_scared(uint32_t b) { return (int)(b & 0xFF); }
__device__ __forceinline__ int rc_carry(uint32_t b) { return (int)((b >> 8) & 0xFFF); }
__device__ __forceinline__ int rc_ret(uint32_t b) { return (int)((b >> 20) & 0xFFF); }

// the one place deaths are decided in this file: bit i set = agent i died in X -> Y, made by mover M
template <int M>
__device__ __forceinline__ int rec_deaths(const RecState &X, const RecState &Y)
{
    int mask = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i == M) continue;
        const bool died = (Y.a[i] & 0xFFFFu) != (X.a[i] & 0xFFFFu) || (rc_scared(X.b[i]) > 0 && rc_scared(Y.b[i]) == 0) ||
                          rc_carry(Y.b[i]) < rc_carry(X.b[i]);
        mask |= died ? 1 << i : 0;
    }
    const int dist = abs(rc_x(Y.a[M]) - rc_x(X.a[M])) + abs(rc_y(Y.a[M]) - rc_y(X.a[M]));
    const bool died = dist > 1 || (rc_carry(Y.b[M]) < rc_carry(X.b[M]) && rc_ret(Y.b[M]) == rc_ret(X.b[M])) ||
                      (rc_scared(X.b[M]) >= 2 && rc_scared(Y.b[M]) == 0);
    return mask | (died ? 1 << M : 0);
}

// EVENT of the sub-step X -> Y made by mover M (the table of include/pmx.h)
template <int M>
__device__ __forceinline__ int32_t rec_event(const RecState &X, const RecState &Y)
{
    const int deaths = rec_deaths<M>(X, Y);
    const bool died = (deaths >> M) & 1;
    const int x = rc_x(X.a[M]), y = rc_y(X.a[M]);
    int move;
    if (!died) {                        // at most one step: the direction of pos_Y - pos_X
        const int dx = rc_x(Y.a[M]) - x, dy = rc_y(Y.a[M]) - y;
        move = dy > 0 ? 0 : dx > 0 ? 1 : dy < 0 ? 2 : dx < 0 ? 3 : 4;
    } else {                            // sent home: the one direction that led onto an enemy of X, if there is exactly one
        constexpr int E1 = (M + 1) & 3, E2 = (M + 3) & 3;
        const int e1x = rc_x(X.a[E1]), e1y = rc_y(X.a[E1]), e2x = rc_x(X.a[E2]), e2y = rc_y(X.a[E2]);
        int n = 0;
        move = 7;
#pragma unroll
        for (int d = 0; d < 5; ++d) {
            const int cx = x + (d == 1) - (d == 3), cy = y + (d == 0) - (d == 2);
            if ((cx == e1x && cy == e1y) || (cx == e2x && cy == e2y)) { move = d; ++n; }
        }
        if (n != 1) move = 7;
    }
    const int ret = rc_ret(Y.b[M]) - rc_ret(X.b[M]);
    return (int32_t)(move | (died ? 8 : 0) | ((deaths & ~(1 << M)) << 4) | (rc_carry(Y.b[M]) > rc_carry(X.b[M]) ? 1 << 8 : 0) |
                     (rec_caps(X) > rec_caps(Y) ? 1 << 9 : 0) | ((ret & 0xFFF) << 10));
}

struct PmxRecordParams {
    const uint32_t *snap[4];     // the states after sub-steps 0, 1, 2 and the current state
    const uint8_t *done;         // [N] or NULL
    const int32_t *layout_idx;   // [N] or NULL (init only)
    int32_t *head;               // [PMX_RECORD_HEAD_WORDS][count]
    int32_t *frames;             // [1 + 4 max_ticks][FW][count]
    int32_t N, first, count, lay_H, max_ticks;
};

// F: word 0 of the frame in this lane's row
__device__ __forceinline__ void rec_store_words(int32_t *F, size_t C, const RecState &s, int32_t score, int32_t event)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        F[(size_t)i * C] = (int32_t)s.a[i];
        F[(size_t)(4 + i) * C] = (int32_t)s.b[i];
    }
    F[(size_t)8 * C] = (int32_t)s.cap[0];
    F[(size_t)9 * C] = (int32_t)s.cap[1];
    F[(size_t)PMX_RECORD_W_SCORE * C] = score;
    F[(size_t)PMX_RECORD_W_EVENT * C] = event;
}

__global__ __launch_bounds__(PMX_RULE_BLOCK) void pmx_game_record_init_kernel(PmxRecordParams p)
{
    const long row = (long)blockIdx.x * PMX_RULE_BLOCK + threadIdx.x;
    if (row >= p.count) return;
    const size_t env = (size_t)(row + p.first), N = (size_t)p.N, C = (size_t)p.count;
    const int H = p.lay_H;
    const uint32_t *S = p.snap[3] + env;
    const RecState cur = rec_load_snap(S, H, N);
    const int32_t score = (int32_t)S[(size_t)PMX_W_SCORE(H) * N];
    const int32_t layout = p.layout_idx ? p.layout_idx[env] : 0;
    int32_t *R = p.head + row, *F = p.frames + row;
#pragma unroll
    for (int w = 0; w < PMX_RECORD_HEAD_WORDS; ++w) R[(size_t)w * C] = w == RH_LAYOUT ? layout : 0;
    rec_store_words(F, C, cur, score, 0);
    for (int y = 0; y < H; ++y) F[(size_t)(PMX_RECORD_W_FOOD + y) * C] = (int32_t)S[(size_t)y * N];
}

// HB: the food rows of the four states are held in registers, HB >= H of them per state
template <int HB>
__global__ __launch_bounds__(PMX_RULE_BLOCK) void pmx_game_record_kernel(PmxRecordParams p)
{
    const long row = (long)blockIdx.x * PMX_RULE_BLOCK + threadIdx.x;
    if (row >= p.count) return;
    const size_t env = (size_t)(row + p.first), N = (size_t)p.N, C = (size_t)p.count;
    const int H = p.lay_H;
    int32_t *R = p.head + row;
    const int32_t len = R[(size_t)RH_LEN * C], was_done = R[(size_t)RH_DONE * C], overflow = R[(size_t)RH_OVERFLOW * C];
    if ((was_done | overflow) != 0) return;                           // a frozen row keeps every word
    if (len < 0 || len >= p.max_ticks) {                              // the log is full (or LEN is not one this kernel wrote)
        R[(size_t)RH_OVERFLOW * C] = 1;
        return;
    }
    const size_t FW = (size_t)PMX_RECORD_FW(H);
    int32_t *F = p.frames + (size_t)(4 * (size_t)len) * FW * C + row;   // frame 4 LEN: X of sub-step 0; the new frames follow it
    // every remaining load of the lane before the first use
    RecState prev;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        prev.a[i] = (uint32_t)F[(size_t)i * C];
        prev.b[i] = (uint32_t)F[(size_t)(4 + i) * C];
    }
    prev.cap[0] = (uint32_t)F[(size_t)8 * C];
    prev.cap[1] = (uint32_t)F[(size_t)9 * C];
    const int32_t prev_score = F[(size_t)PMX_RECORD_W_SCORE * C];
    const uint8_t done = p.done ? p.done[env] : (uint8_t)0;
    RecState s[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) s[m] = rec_load_snap(p.snap[m] + env, H, N);
    const int32_t score = (int32_t)p.snap[3][(size_t)PMX_W_SCORE(H) * N + env];
    uint32_t food[4][HB];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int y = 0; y < HB; ++y) food[m][y] = y < H ? p.snap[m][(size_t)y * N + env] : 0u;
    int32_t ev[4];
    ev[0] = rec_event<0>(prev, s[0]);
    ev[1] = rec_event<1>(s[0], s[1]);
    ev[2] = rec_event<2>(s[1], s[2]);
    ev[3] = rec_event<3>(s[2], s[3]);
    // the snapshots carry no score word: only the mover's returned pellets move the score (red up, blue down), so the score
    // after sub-steps 0 .. 2 follows from the previous frame's; after sub-step 3 it is the state's own word
    int32_t sc[4];
    sc[0] = prev_score + (rc_ret(s[0].b[0]) - rc_ret(prev.b[0]));
    sc[1] = sc[0] - (rc_ret(s[1].b[1]) - rc_ret(s[0].b[1]));
    sc[2] = sc[1] + (rc_ret(s[2].b[2]) - rc_ret(s[1].b[2]));
    sc[3] = score;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        int32_t *G = F + (size_t)(1 + m) * FW * C;
        rec_store_words(G, C, s[m], sc[m], ev[m]);
#pragma unroll
        for (int y = 0; y < HB; ++y)
            if (y < H) G[(size_t)(PMX_RECORD_W_FOOD + y) * C] = (int32_t)food[m][y];
    }
    R[(size_t)RH_LEN * C] = len + 1;
    R[(size_t)RH_DONE * C] = done != 0 ? 1 : 0;
}

// count > 0 rows, 1 <= H <= 32, max_ticks >= 1; ev0 / ev1 as in pmx_launch_episode_stats (the update only)
extern "C" hipError_t pmx_launch_game_record(const uint32_t *const *snap, const uint8_t *done, const int32_t *layout_idx, int32_t *head,
                                             int32_t *frames, int N, int first, int count, int H, int max_ticks, int init, hipStream_t st,
                                             hipEvent_t ev0, hipEvent_t ev1)
{
    PmxRecordParams p;
    for (int a = 0; a < 4; ++a) p.snap[a] = snap[a];
    p.done = done;
    p.layout_idx = layout_idx;
    p.head = head;
    p.frames = frames;
    p.N = N, p.first = first, p.count = count, p.lay_H = H, p.max_ticks = max_ticks;
    const dim3 grid((unsigned)(((long)count + PMX_RULE_BLOCK - 1) / PMX_RULE_BLOCK)), block(PMX_RULE_BLOCK);
    if (init) {
        hipLaunchKernelGGL(pmx_game_record_init_kernel, grid, block, 0, st, p);
        return hipGetLastError();
    }
#define PMX_RECORD_LAUNCH(HB)                                                                                          \
    do {                                                                                                               \
        if (ev0) hipExtLaunchKernelGGL((pmx_game_record_kernel<HB>), grid, block, 0, st, ev0, ev1, 0, p);              \
        else hipLaunchKernelGGL((pmx_game_record_kernel<HB>), grid, block, 0, st, p);                                  \
    } while (0)
    if (H <= 12) PMX_RECORD_LAUNCH(12);
    else if (H <= 16) PMX_RECORD_LAUNCH(16);
    else if (H <= 20) PMX_RECORD_LAUNCH(20);
    else PMX_RECORD_LAUNCH(32);
#undef PMX_RECORD_LAUNCH
    return hipGetLastError();
}
