"""CPU suite of the in-kernel approxQTeam: the C ABI of the new entry point, the Python restatement of the bots
(tests/_approxq_model.py) against the reference's own numbers (fixture G10), the fixture's coverage, and the trainer's
`hard_bots` draws on a stand-in env.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _approxq_model as AQ
import _golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ("small", "tiny", "blox")
# what the issue requires of the offensive records of every layout (counted as make_golden_approxq.py counts)
COVERAGE = dict(g_ge1=50, g_eq2=10, eats=50, home=50, home_12=20, ties=50)


def test_bot_query_abi():
    import pmx
    L = pmx._lib
    assert L.ACTION_APPROXQ_OFFENSE == -5 and L.ACTION_APPROXQ_DEFENSE == -6
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pmx.h")).read(), flags=re.S)
    m = re.search(r"int\s+pmx_bot_query\s*\(([^)]*)\)", src)
    assert m, "include/pmx.h does not declare pmx_bot_query"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 7 and params[1].startswith("int ") and params[2].startswith("int ")
    assert "double" in params[3] and "int8_t" in params[4] and "uint8_t" in params[5]
    assert re.search(r"#define\s+PMX_ACTION_APPROXQ_OFFENSE\s+\(-5\)", src) and re.search(r"#define\s+PMX_ACTION_APPROXQ_DEFENSE\s+\(-6\)", src)
    proto = {n: (r, a) for n, r, a in L.PROTOTYPES}
    assert proto["pmx_bot_query"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    lib = L.load()
    assert lib.pmx_bot_query(None, 0, -5, None, None, None, None) == -1
    assert b"null" in lib.pmx_last_error()
    assert lib.pmx_version() == 1


def _records(lay):
    d, meta = G.load(f"approxq_{lay}.npz")
    states = AQ.states_from_arrays(*(d["in_" + k] for k in ("pos", "dir", "pac", "scared", "carry", "ret", "food", "caps", "score", "steps")))
    return d, meta, states


@pytest.mark.parametrize("lay", LAYOUTS)
def test_model_equals_reference_on_every_record(lay):
    """Every G10 record: legal mask, values (as bytes: the float64 Q sum must round like the reference's), the features
    behind them, food left, best set and the walk-home action."""
    d, meta, states = _records(lay)
    model = AQ.Model(meta["layout"])
    pst = AQ.to_pstates(states)
    n = len(d["state"])
    assert n >= 4 * 700
    for k in range(n):
        s, i = int(d["state"][k]), int(d["agent"][k])
        code = AQ.AQ_OFF if d["offense"][k] else AQ.AQ_DEF
        assert bool(d["offense"][k]) == (i < 2)
        ev = model.evaluate(states[s], i, code, pst[s])
        assert ev["legal"] == d["legal"][k], k
        assert ev["values"].tobytes() == d["values"][k].tobytes(), (k, ev["values"], d["values"][k])
        assert ev["food_left"] == d["food_left"][k] and ev["best"] == d["best"][k] and ev["home"] == d["home"][k], k
        if d["offense"][k]:
            for name in ("g", "eats", "d"):
                assert (ev[name] == d[name][k]).all(), (k, name)


@pytest.mark.parametrize("lay", LAYOUTS)
def test_fixture_coverage_and_drop_share(lay):
    d, meta, _ = _records(lay)
    off = d["offense"] == 1
    legal = ((d["legal"][:, None] >> np.arange(5)[None]) & 1).astype(bool)
    gmax = np.where(legal, d["g"], -1).max(1)
    ties = np.array([bin(int(b)).count("1") > 1 for b in d["best"]])
    cov = dict(g_ge1=int((gmax >= 1)[off].sum()), g_eq2=int((gmax == 2)[off].sum()), eats=int(((d["eats"] == 1).any(1))[off].sum()),
               home=int((d["food_left"] <= 2)[off].sum()), home_12=int(((d["food_left"] >= 1) & (d["food_left"] <= 2))[off].sum()),
               ties=int(ties[off].sum()))
    print(lay, cov, "dropped", meta["dropped"], "of", meta["n_states"])
    for k, need in COVERAGE.items():
        assert cov[k] >= need, (k, cov[k], need)
        assert cov[k] == meta["coverage"][k]
    assert (d["agent"][off] == 0).any() and (d["agent"][off] == 1).any()
    assert meta["dropped"] <= 0.02 * meta["n_states"]
    assert ((d["home"] >= 0) == (d["food_left"] <= 2)).all()


def test_draws_of_the_model():
    """The hash is random_legal's (salt 0) and bot_action's (salt 0x5bd1e995) generator; the explore threshold is
    ceil(2^32 / 10); picks walk the list order N, S, E, W, Stop."""
    assert AQ.lowbias32(0) == 0                      # (the constants are pinned by the GPU differential test)
    assert 0x1999999A == -(-2 ** 32 // 10)
    assert AQ.pick(0b11111, 0) == 0 and AQ.pick(0b11111, 2 ** 32 - 1) == 4
    assert [AQ.pick(0b10110, x << 30) for x in range(4)] == [2, 2, 1, 4]
    share = np.mean([AQ.h(7, e, t, 0, AQ.SALT_EXPLORE) < 0x1999999A for e in range(200) for t in range(50)])
    assert abs(share - 0.1) < 5 * (0.09 / 10000) ** 0.5
    ev = dict(legal=0b10011, best=0b00010, home=-1)
    acts = [AQ.Model.play(ev, AQ.AQ_OFF, 3, e, 11, 2) for e in range(400)]
    assert all(a == 1 for a, f in acts if f == 0) and {f for _, f in acts} == {0, AQ.FLAG_EXPLORED}
    assert all(a == AQ.pick(0b10011, AQ.h(3, e, 11, 2, 0)) for e, (a, f) in enumerate(acts) if f)
    assert AQ.Model.play(dict(legal=0b10011, best=0b00010, home=4), AQ.AQ_OFF, 3, 0, 11, 2) == (4, AQ.FLAG_HOME)


# ---- the trainer's opponent schedule on a stand-in env (the stub of tests/test_mappo_cpu.py) --------------------------
class _StubEnv:
    def __init__(self, layout, n_envs):
        from pmx.layout import get_layout
        self.layout = get_layout(layout)
        self.obs_torch_dtype = torch.float32
        self.n_envs = n_envs

    def reset(self):
        return torch.zeros((self.n_envs, 4, 8, self.layout.height, self.layout.width)), None

    def close(self):
        pass


def _trainer(**kw):
    from pmx import trainer
    return trainer.VecMAPPOTrainer("tinyCapture", 4, horizon=2, minibatch=8, device="cpu", seed=1, use_autocast=False,
                                   opponent="curriculum", curriculum_scale=0.1, total_updates=40, env=_StubEnv("tinyCapture", 4), **kw)


def _draws(tr, per_phase=200):
    out = []
    for idx in (10, 50, 200):
        for _ in range(per_phase):
            tr.update_idx = idx
            out.append(tr._pick_opponent())
    return out


def test_hard_bots_draws_and_checkpoint(tmp_path):
    a, b = _trainer(), _trainer(hard_bots=("baseline",))
    da = _draws(a)
    assert da == _draws(b) and len(da) == 600
    assert {m for m, _ in da} == {"random", "baseline", "self", "pool"}
    c = _trainer(hard_bots=("baseline", "approxq"))
    dc = _draws(c)
    p1, p2, p3 = ({m for m, _ in dc[k:k + 200]} for k in (0, 200, 400))
    assert p1 == {"random"} and p2 == {"random", "baseline", "approxq"} and p3 == {"self", "pool", "random", "baseline", "approxq"}
    with pytest.raises(ValueError):
        _trainer(hard_bots=("astar",))
    # save_full / load_full carry hard_bots and the stream of draws
    path = str(tmp_path / "full.pt")
    c.save_full(path)
    ck = torch.load(path, weights_only=True)
    assert ck["hard_bots"] == ["baseline", "approxq"]
    e = _trainer()
    e.load_full(path)
    assert e.hard_bots == ("baseline", "approxq")
    assert _draws(c, 40) == _draws(e, 40)
    # a file written before hard_bots existed loads with the default
    del ck["hard_bots"]
    torch.save(ck, path)
    f = _trainer(hard_bots=("approxq",))
    f.load_full(path)
    assert f.hard_bots == ("baseline",)


def test_host_team_file_roles():
    from pmx.capture_agents import load_agents
    red = load_agents(True, "approxQTeam")
    blue = load_agents(False, "approxQTeam")
    assert [a.index for a in red] == [0, 2] and [a.index for a in blue] == [1, 3]
    assert type(red[0]).__name__ == "QForager" and red[1].home_at == 2
    base = load_agents(True, "baselineTeam")
    assert base[0].home_at == 0 and base[1].home_at == 0
