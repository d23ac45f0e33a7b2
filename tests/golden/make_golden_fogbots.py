#!/usr/bin/env python3
"""Generate the fog-bound-bot fixtures under tests/golden/ by IMPORTING the reference (see make_golden.py, whose helpers this
script uses; like it, it runs only where the reference is present and copies nothing of it: numbers only).

Usage:
    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_fogbots.py [section ...]
sections: fogbots traces   (default: both)

  G12 fogbots.npz   the reference's baselineTeam and approxQTeam agents asked on the CONTEST'S observation of the states of
        G11's rows (fog_sight.npz; a row names a record of an existing fixture and an observer).  Per row the GameState is
        rebuilt, agents of both team files with the observer's index are registered, obs = agent.observationFunction(state) is
        taken under random.seed(k) (G11's k) and, per legal action, evaluate(obs, action) (the reflex roles) or
        getQValue(obs, action) (the forager) is recorded as float64 (NaN where illegal), with the best set, the walk-home
        action (-1 where the role does not walk home) and the two seen flags (enemy with the lower index first).  One block at
        the contest's SIGHT_RANGE = 5 and one with capture.SIGHT_RANGE = 1 assigned before the calls, where alone the forager's
        ghost count can change.  Every row for the role / sight pairs where the rule bites (the defenders at sight 5, the
        forager at sight 1), every CONTROL_STRIDE-th row for the others (the forager at sight 5 and the offensive reflex agent
        at both sights must equal their full-state values; the defenders at sight 1).  For the forager g_obs / g_full hold the
        reference's own ghost feature (its extractor's "#-of-ghosts-1-step-away" times ten) per action on the observation and on
        the full state.
  G9  bots_small_baselineTeam_fog.json, bots_blox_approxQTeam_fog.json   section_bots' recipe (make_golden.py) with blue played by its scripted Hunter, and each red
        bot instance's getAction wrapped to go through its own observationFunction, as a contest game asks it; hidden_turns
        counts the defender's turns outside the walk home in which an invader was hidden from it (the turns the rule can change),
        hidden_turns_any_bot those of both bots, walks home included.
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
import capture                    # noqa: E402  (the reference's)

OUT = MG.OUT
STATE_KEYS = ("pos", "dir", "pac", "scared", "carry", "ret", "food", "caps", "score")
BASE_OFF, BASE_DEF, AQ_OFF, AQ_DEF = -3, -4, -5, -6
CONTROL_STRIDE = 8
# (sight, code, stride over G11's rows)
BLOCKS = ((5, BASE_DEF, 1), (5, AQ_DEF, 1), (1, AQ_OFF, 1),
          (5, AQ_OFF, CONTROL_STRIDE), (5, BASE_OFF, CONTROL_STRIDE), (1, BASE_OFF, CONTROL_STRIDE),
          (1, BASE_DEF, CONTROL_STRIDE), (1, AQ_DEF, CONTROL_STRIDE))
HOME_AT = {BASE_OFF: 0, BASE_DEF: 0, AQ_OFF: 2, AQ_DEF: 2}
MIN_HIDDEN_SHARE, MIN_BOTH, MIN_G_DIFFERS, MAX_DROP_SHARE = 0.05, 5, 40, 0.03
CALL_SECONDS = 4
MIN_HIDDEN_TURNS = 10


def load_team(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(MG.REF, "agents", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ghost_count(agent, gs, action):
    """The reference's own ghost feature of (gs, action): its extractor divides every feature by ten."""
    tenth = agent.featuresExtractor.getFeatures(gs, action)["#-of-ghosts-1-step-away"]
    g = int(round(tenth * 10.0))
    assert g in (0, 1, 2) and abs(tenth * 10.0 - g) < 1e-9
    return g


def evaluate(agent, code, gs, k):
    """One record: the agent asked on its own observation of gs."""
    i = agent.index
    random.seed(k)
    obs = agent.observationFunction(gs)
    foes = sorted(agent.getOpponents(gs))
    seen = [obs.getAgentPosition(o) is not None for o in foes]
    legal = obs.getLegalActions(i)
    assert legal == gs.getLegalActions(i)
    values = np.full(5, np.nan, np.float64)
    g_obs, g_full = np.full(5, -1, np.int8), np.full(5, -1, np.int8)
    for a in legal:
        c = MG.DIR2INT[a]
        if code == AQ_OFF:
            values[c] = float(agent.getQValue(obs, a))
            g_obs[c], g_full[c] = ghost_count(agent, obs, a), ghost_count(agent, gs, a)
        else:
            values[c] = float(agent.evaluate(obs, a))
    best = np.nanmax(values)
    food_left = len(agent.getFood(obs).asList())
    home = -1
    if food_left <= HOME_AT[code]:
        st = random.getstate()
        home = MG.DIR2INT[agent.chooseAction(obs)]
        assert random.getstate() == st, "the home walk must not draw"
    inv = [bool(gs.getAgentState(o).isPacman) for o in foes]
    return dict(agent=i, legal=MG.legal_mask([MG.DIR2INT[a] for a in legal]), values=values,
                best=MG.legal_mask([c for c in range(5) if values[c] == best]), home=home, seen=seen, food_left=food_left,
                g_obs=g_obs, g_full=g_full, hidden_inv=any(v and not s for v, s in zip(inv, seen)),
                both_inv=any(v and not s for v, s in zip(inv, seen)) and any(v and s for v, s in zip(inv, seen)))


def section_fogbots():
    print("G12 fog-bound bot evaluations")
    z11 = np.load(os.path.join(OUT, "fog_sight.npz"))
    meta11 = json.loads(bytes(z11["meta"]).decode())
    assert meta11["sight_range"] == capture.SIGHT_RANGE == 5
    base, aq = load_team("baselineTeam"), load_team("approxQTeam")
    signal.signal(signal.SIGALRM, MG._alarm)
    recs, per_source = [], {}
    for s, name in enumerate(meta11["sources"]):
        lay = name.split("_")[1]                    # scen_small_random.npz -> small
        z = np.load(os.path.join(OUT, name))
        env = MG.make_env(lay, 300)
        MG.quiet(env.reset)
        agents = {}
        for i in range(4):
            b, q = base.createTeam(i, i, i % 2 == 0), aq.createTeam(i, i, i % 2 == 0)
            agents[i] = {BASE_OFF: b[0], BASE_DEF: b[1], AQ_OFF: q[0], AQ_DEF: q[1]}
            for ag in agents[i].values():
                MG.quiet(ag.registerInitialState, env.game.state)
        rows = np.flatnonzero(z11["src"] == s)
        n_drop, first = 0, len(recs)
        for n, r in enumerate(rows):
            idx, sub, observer = int(z11["idx"][r]), int(z11["sub"][r]), int(z11["observer"][r])
            st = {key: (z["in_" + key][idx] if sub < 0 else z["sub_" + key][idx, sub]) for key in STATE_KEYS}
            MG.inject(env, dict(st, steps=0))
            gs = env.game.state
            mine = []
            signal.alarm(CALL_SECONDS)
            try:
                for sight, code, stride in BLOCKS:
                    if n % stride:
                        continue
                    capture.SIGHT_RANGE = sight
                    rec = MG.quiet(evaluate, agents[observer][code], code, gs, int(z11["k"][r]))
                    rec.update(row=int(r), code=code, sight=sight)
                    mine.append(rec)
            except AssertionError:               # a condition of this generator: never a dropped state
                raise
            except (MG._Timeout, Exception):     # the reference raises on states its successor generation cannot handle
                n_drop += 1
                continue
            finally:
                signal.alarm(0)
                capture.SIGHT_RANGE = 5
            foes = [o for o in range(4) if o % 2 != observer % 2]
            for rec in mine:                     # the seen flags at the contest's range are G11's
                assert rec["sight"] != 5 or rec["seen"] == [bool(z11["vis"][r][o]) for o in foes], r
            recs += mine
        mine = recs[first:]
        d5 = [r for r in mine if r["sight"] == 5 and r["code"] == BASE_DEF]
        per_source[name] = dict(rows=int(len(rows)), dropped=n_drop, hidden=sum(r["hidden_inv"] for r in d5),
                                both=sum(r["both_inv"] for r in d5), defender_records=len(d5))
        print(f"  {name}: {per_source[name]}", flush=True)
        assert n_drop <= MAX_DROP_SHARE * len(rows), (name, n_drop)
        assert per_source[name]["hidden"] >= MIN_HIDDEN_SHARE * len(d5), name
        assert per_source[name]["both"] >= MIN_BOTH, name
    differs = sum(r["sight"] == 1 and r["code"] == AQ_OFF and bool((r["g_obs"] != r["g_full"]).any()) for r in recs)
    print(f"  forager records at sight 1 whose ghost count differs from the full state's: {differs} (synthesised: 0)", flush=True)
    assert differs >= MIN_G_DIFFERS, differs
    for r in recs:                          # the controls equal the full-state values by construction of the rule
        if r["code"] == AQ_OFF and r["sight"] == 5:
            assert (r["g_obs"] == r["g_full"]).all()
    data = dict(row=np.array([r["row"] for r in recs], np.int32), code=np.array([r["code"] for r in recs], np.int8),
                sight=np.array([r["sight"] for r in recs], np.uint8), agent=np.array([r["agent"] for r in recs], np.uint8),
                legal=np.array([r["legal"] for r in recs], np.uint8), values=np.stack([r["values"] for r in recs]),
                best=np.array([r["best"] for r in recs], np.uint8), home=np.array([r["home"] for r in recs], np.int8),
                seen=np.array([r["seen"] for r in recs], np.uint8), food_left=np.array([r["food_left"] for r in recs], np.int16),
                g_obs=np.stack([r["g_obs"] for r in recs]), g_full=np.stack([r["g_full"] for r in recs]))
    meta = dict(per_source=per_source, g_differs=int(differs), synthesised=0, control_stride=CONTROL_STRIDE,
                blocks=[list(b) for b in BLOCKS], min_hidden_share=MIN_HIDDEN_SHARE, min_both=MIN_BOTH, min_g_differs=MIN_G_DIFFERS,
                source="agents/baselineTeam.py and agents/approxQTeam.py createTeam(i, i, i % 2 == 0) on obs = "
                       "agent.observationFunction(state) under random.seed(k): evaluate / getQValue / chooseAction; "
                       "the sight-1 block with capture.SIGHT_RANGE = 1 assigned by the generator")
    data["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    path = os.path.join(OUT, "fogbots.npz")
    np.savez_compressed(path, **data)
    print(f"  fogbots.npz: records {len(recs)} size={os.path.getsize(path)}", flush=True)
    assert os.path.getsize(path) <= 200 * 1000


def _hook(env, chosen, hidden, home_at):
    """Every red bot instance is asked through its own observationFunction, as capture.py's game loop asks it.  hidden gets one
    pair per bot turn: (an invader of the bot's side is hidden from it, the turn is one the rule can change: the bot is the
    team's defender and does not walk home -- at sight 5 the forager's ghost count never changes, see G12)."""
    for b in (env.agents[0], env.agents[2]):
        if getattr(b, "_fog_wrapped", False):       # reset() keeps the instances
            continue
        b._fog_wrapped = True
        orig = b.getAction

        def wrap(gs, _o=orig, _b=b):
            obs = _b.observationFunction(gs)
            hid = any(gs.getAgentState(o).isPacman and obs.getAgentPosition(o) is None for o in _b.getOpponents(gs))
            acts = type(_b).__name__ == "DefensiveReflexAgent" and len(_b.getFood(gs).asList()) > home_at
            hidden.append((hid, hid and acts))
            a = _o(obs)
            chosen.append(a)
            return a
        b.getAction = wrap


def section_traces():
    print("G9 fog-bound bot traces")
    for lay, team, seed, ticks in (("small", "baselineTeam", 11, 320), ("blox", "approxQTeam", 13, 320)):
        random.seed(seed)
        env = MG.make_env(lay, 299, self_play=False, enemy=team)
        rng = np.random.RandomState(1)
        MG.quiet(env.reset)
        chosen, hidden = [], []
        _hook(env, chosen, hidden, HOME_AT[AQ_DEF if team == "approxQTeam" else BASE_DEF])
        hunter = MG.Hunter(env, rng, 0.15)          # blue has to invade for the rule to bite: make_golden.py's scripted policy
        trace, scores, rewards, dones, blue = [], [], [], [], []
        for t in range(ticks):
            gs = env.game.state
            a1, a3 = (hunter.act(i, [MG.DIR2INT[a] for a in gs.getLegalActions(i)]) for i in (1, 3))
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
                _hook(env, chosen, hidden, HOME_AT[AQ_DEF if team == "approxQTeam" else BASE_DEF])
        n_all, n_hidden = int(sum(h for h, _ in hidden)), int(sum(a for _, a in hidden))
        assert n_hidden >= MIN_HIDDEN_TURNS, (lay, team, n_hidden, n_all)
        with open(os.path.join(OUT, f"bots_{lay}_{team}_fog.json"), "w") as f:
            json.dump(dict(layout=MG.layout_text(lay), team=team, random_seed=seed, length=299, blue_actions=blue,
                           red_actions=trace, scores=scores, rewards=rewards, dones=dones, hidden_turns=n_hidden, hidden_turns_any_bot=n_all, fog_bots=True,
                           source="gymPacMan_parallel_env(self_play=False, enemieName=team); random.seed(k) before ctor; "
                                  "blue = make_golden.Hunter(env, numpy RandomState(1), 0.15) on the tick-start state; each red bot's getAction wrapped to "
                                  "receive its own observationFunction(state)"), f)
        print(f"  bots_{lay}_{team}_fog.json defender turns outside the walk home with a hidden invader {n_hidden} (any bot turn: {n_all}) final scores {sorted(set(scores))[:6]} dones={sum(dones)}", flush=True)


SECTIONS = dict(fogbots=section_fogbots, traces=section_traces)

if __name__ == "__main__":
    for s in sys.argv[1:] or ["fogbots", "traces"]:
        SECTIONS[s]()
