#!/usr/bin/env python3
"""Generate the approxQTeam fixtures under tests/golden/ by IMPORTING the reference (see make_golden.py, whose helpers
this script uses; like it, it runs only where the reference is present and copies nothing of it).

Usage:
    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_approxq.py [section ...]
sections: approxq bots score   (default: approxq bots)

  G10 approxq_{small,tiny,blox}.npz   agents/approxQTeam.py evaluated on synthesized and played states, both colours:
        per record (one agent of one state) the legal mask, getQValue / evaluate of every legal action as float64 (NaN
        where illegal), the food left on the attacked side, the best-action mask, the home-walk action where
        food_left <= 2 (else -1), and for the offensive role the three features behind the Q value
        (g = ghosts one step away, eats, d = steps to the closest pellet, -1 = feature absent).
  G9  bots_{small,tiny}_approxQTeam.json   section_bots' recipe with team="approxQTeam".
  score (prints only)   mean final score of the reference's approxQTeam (red) against uniformly random blue actions.
"""
import importlib.util
import json
import os
import random
import signal
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG          # noqa: E402  (puts the reference on sys.path and chdirs to a scratch directory)
from game import Actions          # noqa: E402

OUT = MG.OUT
N_RANDOM, N_PLAYED, SEED = 400, 400, 7
CALL_SECONDS = 4                  # per state (four agents x five actions take milliseconds where the reference ends)
# coverage the offensive records of every layout must reach (the generator and tests/test_approxq_cpu.py assert them)
COVERAGE = dict(g_ge1=50, g_eq2=10, eats=50, home=50, home_12=20, ties=50)
MAX_DROP_SHARE = 0.02


def load_team():
    spec = importlib.util.spec_from_file_location("ref_approxQTeam", os.path.join(MG.REF, "agents", "approxQTeam.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def played_states(lay, n, seed):
    """States met in play: the reference's approxQTeam (red) against random blue actions, one snapshot per tick."""
    random.seed(seed)
    env = MG.make_env(lay, 299, self_play=False, enemy="approxQTeam")
    rng = np.random.RandomState(seed)
    MG.quiet(env.reset)
    out = []
    while len(out) < n:
        st = {k: np.array(v) for k, v in MG.snapshot(env.game.state).items()}
        st["steps"] = int(env.steps)
        st["name"] = f"play{len(out)}"
        out.append(st)
        _, _, term, _ = env.step({env.agents[1]: int(rng.randint(5)), env.agents[3]: int(rng.randint(5))})
        if any(term.values()):
            MG.quiet(env.reset)
    return out


def evaluate_agent(agent, gs, offense):
    idx = agent.index
    legal = gs.getLegalActions(idx)
    rec = dict(agent=idx, offense=int(offense), legal=MG.legal_mask([MG.DIR2INT[a] for a in legal]))
    values = np.full(5, np.nan, np.float64)
    g = np.full(5, -1, np.int8)
    eats = np.full(5, -1, np.int8)
    d = np.full(5, -1, np.int16)
    for a in legal:
        c = MG.DIR2INT[a]
        if offense:
            values[c] = float(agent.getQValue(gs, a))
            food = agent.getFood(gs)
            walls = gs.getWalls()
            x, y = gs.getAgentPosition(idx)
            dx, dy = Actions.directionToVector(a)
            nx, ny = int(x + dx), int(y + dy)
            ghosts = [s.getPosition() for s in (gs.getAgentState(i) for i in agent.getOpponents(gs)) if not s.isPacman]
            g[c] = sum((nx, ny) in Actions.getLegalNeighbors(p, walls) for p in ghosts)
            eats[c] = int(g[c] == 0 and bool(food[nx][ny]))
            dist = agent.featuresExtractor.closestFood((nx, ny), food, walls)
            d[c] = -1 if dist is None else dist
        else:
            values[c] = float(agent.evaluate(gs, a))
    best = np.nanmax(values)
    rec["values"] = values
    rec["best"] = MG.legal_mask([c for c in range(5) if values[c] == best])
    rec["food_left"] = len(agent.getFood(gs).asList())
    rec["home"] = -1
    if rec["food_left"] <= 2:
        st = random.getstate()
        rec["home"] = MG.DIR2INT[agent.chooseAction(gs)]
        assert random.getstate() == st, "the home walk must not draw"
    rec["g"], rec["eats"], rec["d"] = g, eats, d
    return rec


def coverage(recs):
    off = [r for r in recs if r["offense"]]
    gmax = [max(int(r["g"][c]) for c in range(5) if (r["legal"] >> c) & 1) for r in off]
    return dict(g_ge1=sum(v >= 1 for v in gmax), g_eq2=sum(v == 2 for v in gmax),
                eats=sum(any(r["eats"][c] == 1 for c in range(5)) for r in off),
                home=sum(r["food_left"] <= 2 for r in off), home_12=sum(1 <= r["food_left"] <= 2 for r in off),
                ties=sum(bin(r["best"]).count("1") > 1 for r in off),
                red=sum(r["agent"] == 0 for r in off), blue=sum(r["agent"] == 1 for r in off))


def section_approxq():
    print("G10 approxQTeam evaluations")
    team_mod = load_team()
    signal.signal(signal.SIGALRM, MG._alarm)
    for lay in ("small", "tiny", "blox"):
        states, _ = MG.random_states(lay, N_RANDOM, SEED, False)
        states += played_states(lay, N_PLAYED, SEED)
        env = MG.make_env(lay, 300)
        MG.quiet(env.reset)
        red = team_mod.createTeam(0, 2, True)
        blue = team_mod.createTeam(1, 3, False)
        for a in red + blue:
            MG.quiet(a.registerInitialState, env.game.state)
        roles = [(red[0], True), (blue[0], True), (red[1], False), (blue[1], False)]
        kept, recs, dropped = [], [], 0
        for st in states:
            MG.inject(env, st)
            gs = env.game.state
            signal.alarm(CALL_SECONDS)
            try:
                mine = [MG.quiet(evaluate_agent, ag, gs, off) for ag, off in roles]
            except (MG._Timeout, Exception):     # the reference raises / never ends on states it cannot handle
                dropped += 1
                continue
            finally:
                signal.alarm(0)
            for r in mine:
                r["state"] = len(kept)
            kept.append(st)
            recs += mine
        cov = coverage(recs)
        print(f"  {lay}: states {len(kept)} dropped {dropped} records {len(recs)} coverage {cov}", flush=True)
        for k, need in COVERAGE.items():
            assert cov[k] >= need, (lay, k, cov[k], need)
        assert cov["red"] > 0 and cov["blue"] > 0
        assert dropped <= MAX_DROP_SHARE * len(states), (lay, dropped)
        data = {}
        for k in ("pos", "dir", "pac", "scared", "carry", "ret", "food", "caps", "score"):
            data["in_" + k] = np.stack([np.asarray(s[k]) for s in kept])
        data["in_steps"] = np.array([int(s.get("steps", 0)) for s in kept], np.int32)
        data["state"] = np.array([r["state"] for r in recs], np.int32)
        data["agent"] = np.array([r["agent"] for r in recs], np.int8)
        data["offense"] = np.array([r["offense"] for r in recs], np.uint8)
        data["legal"] = np.array([r["legal"] for r in recs], np.uint8)
        data["values"] = np.stack([r["values"] for r in recs])
        data["food_left"] = np.array([r["food_left"] for r in recs], np.int32)
        data["best"] = np.array([r["best"] for r in recs], np.uint8)
        data["home"] = np.array([r["home"] for r in recs], np.int8)
        data["g"] = np.stack([r["g"] for r in recs])
        data["eats"] = np.stack([r["eats"] for r in recs])
        data["d"] = np.stack([r["d"] for r in recs])
        meta = dict(layout=MG.layout_text(lay), layout_name=lay, n_states=len(states), dropped=dropped, seed=SEED,
                    coverage=cov, source="agents/approxQTeam.py createTeam(0, 2, True) / createTeam(1, 3, False): getQValue, "
                                         "evaluate, chooseAction on injected GameStates")
        data["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
        path = os.path.join(OUT, f"approxq_{lay}.npz")
        np.savez_compressed(path, **data)
        print(f"  {os.path.basename(path)} size={os.path.getsize(path)}", flush=True)


def _hook(env, chosen):
    for b in (env.agents[0], env.agents[2]):
        orig = b.getAction

        def wrap(gs, _o=orig):
            a = _o(gs)
            chosen.append(a)
            return a
        b.getAction = wrap


def section_bots():
    print("G9 approxQTeam traces")
    team = "approxQTeam"
    for lay, seed, ticks in (("small", 4, 320), ("tiny", 5, 320)):
        random.seed(seed)
        env = MG.make_env(lay, 299, self_play=False, enemy=team)
        rng = np.random.RandomState(1)
        MG.quiet(env.reset)
        chosen = []
        _hook(env, chosen)
        trace, scores, rewards, dones, blue = [], [], [], [], []
        for t in range(ticks):
            a1, a3 = int(rng.randint(5)), int(rng.randint(5))
            blue.append([a1, a3])
            chosen.clear()
            obs, rew, term, info = env.step({env.agents[1]: a1, env.agents[3]: a3})
            trace.append([MG.DIR2INT[c] for c in chosen])
            scores.append(int(env.game.state.data.score))
            rewards.append([float(rew[env.agents[0]]), float(rew[env.agents[1]])])
            d = bool(any(term.values()))
            dones.append(d)
            if d:
                MG.quiet(env.reset)
                _hook(env, chosen)
        with open(os.path.join(OUT, f"bots_{lay}_{team}.json"), "w") as f:
            json.dump(dict(layout=MG.layout_text(lay), team=team, random_seed=seed, length=299, blue_actions=blue,
                           red_actions=trace, scores=scores, rewards=rewards, dones=dones,
                           source="gymPacMan_parallel_env(self_play=False, enemieName=team); random.seed(k) before ctor; "
                                  "blue = numpy RandomState(1).randint(5) x2 per tick"), f)
        print(f"  bots_{lay}_{team}.json final scores {sorted(set(scores))[:6]} dones={sum(dones)}", flush=True)


def section_score(games=20, lay="small"):
    """Mean final score of the reference's approxQTeam (red) against uniformly random legal blue actions, one episode of
    length 300 per seed (the figure DESIGN.md quotes beside the in-kernel team's)."""
    finals = []
    for seed in range(games):
        random.seed(1000 + seed)
        env = MG.make_env(lay, 300, self_play=False, enemy="approxQTeam")
        MG.quiet(env.reset)
        done = False
        while not done:
            gs = env.game.state
            acts = {}
            for i in (1, 3):                      # randomTeam: random.choice of the legal actions (tick-start state)
                acts[env.agents[i]] = MG.DIR2INT[random.choice(gs.getLegalActions(i))]
            _, _, term, _ = env.step(acts)
            done = any(term.values())
        finals.append(int(env.game.state.data.score))
    print(f"score {lay}: approxQTeam (red) vs random legal blue, {games} games: mean {np.mean(finals):.2f} "
          f"min {min(finals)} max {max(finals)} wins {sum(f > 0 for f in finals)}", flush=True)


SECTIONS = dict(approxq=section_approxq, bots=section_bots, score=section_score)

if __name__ == "__main__":
    for s in sys.argv[1:] or ["approxq", "bots"]:
        SECTIONS[s]()
