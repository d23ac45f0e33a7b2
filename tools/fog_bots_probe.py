"""What the bots' sight rule (pmx_set_bot_sight) changes in play: in-kernel baselineTeam against baselineTeam.

Part 1, decisions: one handle at the contest's sight, stepped agent by agent; before every defender's sub-step pmx_bot_query is
asked twice, with the rule on and with it off (same state, same draws), and the rule-on action is played.  Reports the share of
defender decisions with a hidden invader and the share whose action differs from the full-state bot's.
Part 2, outcomes: whole ticks, one episode per env, with the rule off and on: blue's win rate (final score < 0).

    python tools/fog_bots_probe.py [--layouts smallCapture bloxCapture] [--envs 256] [--ticks 300] [--sight 5]
prints one JSON line per layout."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pmx  # noqa: E402

OFFENSE, DEFENSE = -3, -4
SEEN_LO, SEEN_HI = 4, 8


def decisions(layout, n_envs, ticks, sight, seed):
    env = pmx.PmxVecEnv(layout, n_envs, length=ticks, auto_reset=True, bots=True, seed=seed, obs_agents=(0,), obs_dtype="uint8")
    env.reset(want_obs=False)
    env.set_bot_sight(sight)
    n = hidden = differs = differs_hidden = 0
    for _ in range(ticks):
        for agent in range(4):
            code = OFFENSE if agent < 2 else DEFENSE
            if code == DEFENSE:
                _, a_on, flags = env.bot_query(agent, code, want_values=False)
                env.set_bot_sight(None)
                _, a_off, _ = env.bot_query(agent, code, want_values=False)
                env.set_bot_sight(sight)
                st = env.get_state()
                foes = (1, 3) if agent % 2 == 0 else (0, 2)
                pac = torch.tensor([[s.pac[o] for o in foes] for s in st], dtype=torch.bool, device=flags.device)
                seen = torch.stack([(flags & SEEN_LO) != 0, (flags & SEEN_HI) != 0], dim=1)
                hid = (pac & ~seen).any(dim=1)
                diff = a_on != a_off
                n += n_envs
                hidden += int(hid.sum())
                differs += int(diff.sum())
                differs_hidden += int((diff & hid).sum())
            env.step_agent(agent, torch.full((n_envs,), code, dtype=torch.int8, device=env.device), want_obs=False)
    env.close()
    return dict(defender_decisions=n, hidden_invader_share=hidden / n, action_differs_share=differs / n,
                action_differs_share_given_hidden=(differs_hidden / hidden if hidden else None))


def blue_win_rate(layout, n_envs, ticks, sight, seed):
    env = pmx.PmxVecEnv(layout, n_envs, length=ticks, auto_reset=True, bots=True, seed=seed, obs_agents=(0,), obs_dtype="uint8")
    env.reset(want_obs=False)
    env.set_bot_sight(sight)
    acts = torch.empty((n_envs, 4), dtype=torch.int8, device=env.device)
    acts[:, :2], acts[:, 2:] = OFFENSE, DEFENSE
    alive = torch.ones(n_envs, dtype=torch.bool, device=env.device)
    final = torch.zeros(n_envs, dtype=torch.int32, device=env.device)
    for _ in range(ticks + 1):
        _, _, done, info = env.step(acts, want_obs=False)
        d = done.to(torch.bool) & alive
        final = torch.where(d, info["score"], final)
        alive &= ~d
        if not bool(alive.any()):
            break
    env.close()
    return dict(blue_win_rate=float((final < 0).double().mean()), red_win_rate=float((final > 0).double().mean()),
                mean_final_score=float(final.double().mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layouts", nargs="+", default=["smallCapture", "bloxCapture"])
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--sight", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    for lay in a.layouts:
        print(json.dumps(dict(layout=lay, envs=a.envs, ticks=a.ticks, sight=a.sight, **decisions(lay, a.envs, a.ticks, a.sight, a.seed),
                              rule_off=blue_win_rate(lay, a.envs, a.ticks, None, a.seed), rule_on=blue_win_rate(lay, a.envs, a.ticks, a.sight, a.seed))),
              flush=True)


if __name__ == "__main__":
    main()
