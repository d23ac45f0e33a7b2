"""gymPacMan_parallel_env(fog_of_war=True): the dicts under the contest's sight rule and the four noisy distances in the infos,
against a twin without the flag (whose dicts tests/test_gpu_dropin.py pins to the reference) and trainer.fog_obs."""
import random

import numpy as np
import pytest
import torch

from test_gpu_fog_emit import _state

pytestmark = pytest.mark.gpu

SIGHT = 5


def _pos(env):
    st = env._env.get_state(0, 1)[0]
    return np.array([[st.pos[i][0], st.pos[i][1]] for i in range(4)], np.int64)


def _within(readings, pos, i):
    return all(abs(int(readings[j]) - int(np.abs(pos[i] - pos[j]).sum())) <= 6 for j in range(4))


def test_self_play_dicts_are_fog_obs_of_the_twins_and_the_readings_follow_the_distances():
    import pmx
    from pmx import trainer
    fog = pmx.gymPacMan_parallel_env("bloxCapture", self_play=True, fog_of_war=True, sight_range=SIGHT)
    twin = pmx.gymPacMan_parallel_env("bloxCapture", self_play=True)
    subs = []                                                       # the twin's positions right after each sub-step
    orig = twin._env.step_agent

    def record(agent, code, **kw):
        out = orig(agent, code, **kw)
        subs.append(_pos(twin))
        return out
    twin._env.step_agent = record
    of, inf = fog.reset()
    ot, it = twin.reset()
    assert sorted(it) == ["legal_actions"] and sorted(inf) == ["agent_distances", "legal_actions"]
    assert inf["legal_actions"] == it["legal_actions"]
    pos = _pos(twin)
    hidden = 0
    for i in range(4):
        assert torch.equal(of[i], trainer.fog_obs(ot[i], SIGHT)) and of[i].dtype == torch.float32
        assert torch.equal(fog.get_Observation(i), trainer.fog_obs(twin.get_Observation(i), SIGHT))
        assert len(inf["agent_distances"][i]) == 4 and _within(inf["agent_distances"][i], pos, i)
    # on from a hand-built state: agents 0 and 1 two cells apart, the other two on their starts in far corners, so that the rule
    # shows some enemies and hides others
    for env in (fog, twin):
        base = env._env.get_state(0, 1)[0]
        starts = [tuple(int(v) for v in env.layout.starts[i]) for i in range(4)]
        env._env.set_state([_state(pmx, env._env, base, [(9, 7), (11, 7), starts[2], starts[3]])])
        env._cached_state = None
    rng = np.random.RandomState(4)
    noise = set()
    seen = 0
    for t in range(30):
        acts = {i: int(rng.randint(0, 5)) for i in range(4)}
        subs.clear()
        of, rf, tf, inf = fog.step(acts)
        ot, rt, tt, it = twin.step(acts)
        assert rf == rt and tf == tt and inf["legal_actions"] == it["legal_actions"] and inf["score_change"] == it["score_change"], t
        assert sorted(it) == ["legal_actions", "score_change"], t                    # the twin's info has no new key
        assert sorted(inf["agent_distances"]) == [0, 1, 2, 3]
        for i in range(4):
            want = trainer.fog_obs(ot[i], SIGHT)
            assert torch.equal(of[i], want), (t, i)
            hidden += int((ot[i][5] != 0).sum()) - int((want[5] != 0).sum())
            seen += int((want[5] != 0).sum())
            r = inf["agent_distances"][i]
            assert len(r) == 4 and all(isinstance(v, int) for v in r) and _within(r, subs[i], i), (t, i, r)
            noise |= {int(r[j]) - int(np.abs(subs[i][i] - subs[i][j]).sum()) for j in range(4)}
        assert torch.equal(fog.get_Observation(1), trainer.fog_obs(twin.get_Observation(1), SIGHT)), t
    assert hidden > 0 and seen > 0                                                   # the rule hid some enemies and showed others
    assert len(noise) >= 10                                                          # 480 draws of 13 values
    fog.close()
    twin.close()


@pytest.mark.parametrize("k", (0, 7))
def test_the_flag_moves_no_draw_of_the_host_bots(k):
    import pmx

    def run(**kw):
        random.seed(k)
        env = pmx.gymPacMan_parallel_env(self_play=False, enemieName="baselineTeam", **kw)
        env.reset()
        chosen, rewards = [], []
        for b in (env.agents[0], env.agents[2]):
            orig = b.getAction

            def wrap(gs, _o=orig):
                a = _o(gs)
                chosen.append(a)
                return a
            b.getAction = wrap
        rng = np.random.RandomState(k)
        keys = []
        for t in range(40):
            o, r, term, info = env.step({env.agents[1]: int(rng.randint(0, 5)), env.agents[3]: int(rng.randint(0, 5))})
            rewards.append([r[a] for a in env.agents])
            keys.append(sorted(info))
            rewards.append(sorted(term.values()))
            if any(term.values()):                                  # the reference's caller resets right after a done
                _, info = env.reset()
                keys.append(sorted(info) + ["score_change"])
        nxt = random.random()
        env.close()
        return chosen, rewards, nxt, keys

    c1, r1, n1, k1 = run(fog_of_war=True)
    c0, r0, n0, k0 = run()
    assert len(c0) == 80 and c1 == c0                               # the bots' action strings
    assert r1 == r0
    assert n1 == n0                                                 # the next draw of `random`: the flag moved no stream
    assert all(ks == ["legal_actions", "score_change"] for ks in k0) and all("agent_distances" in ks for ks in k1)
