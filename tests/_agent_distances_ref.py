"""pmx_agent_distances of include/pmx.h ("Sight rule on the four-agent planes") restated in numpy: the reading table
r[a][i] = manhattan(P_a[a], P_a[i]) + n, the draw taken from tests/_belief_ref.py (the generator pmx_belief_update uses).  The model
tests/test_obs_sight_cpu.py holds to the reference's readings (fixture G11) and to _belief_ref's, and the GPU tests compare the kernel
with.  Vectorised over n envs."""
import numpy as np

from _belief_ref import manhattan, noise


def readings(P, seed, env, ticks):
    """the agent == -1 form.  P [n, 4 sources, 4 agents, 2]: P[:, a] = the positions in the source agent a's planes are encoded from;
    env [n] env indices; ticks [n] the env's tick counter at the call.  -> [n, 4, 4] int64, r[:, a, i]"""
    P = np.asarray(P).astype(np.int64)
    env, ticks = np.asarray(env), np.asarray(ticks)
    out = np.zeros((len(P), 4, 4), np.int64)
    for a in range(4):
        for i in range(4):
            out[:, a, i] = manhattan(P[:, a, a], P[:, a, i]) + noise(seed, env, ticks, 4 * a + i)
    return out


def readings_agent(P, agent, seed, env, ticks):
    """the agent == 0 .. 3 form.  P [n, 4 agents, 2]: the positions in the current state.  -> [n, 4] int64"""
    P = np.asarray(P).astype(np.int64)
    return np.stack([manhattan(P[:, agent], P[:, i]) + noise(seed, np.asarray(env), np.asarray(ticks), 4 * agent + i) for i in range(4)], 1)
