"""CPU suite: the game records (include/pmx.h, "Game records") as the plain-numpy model of _game_record_ref.py states them, on the
recorded sub-step states of the golden trajectories and on mid-game states stepped by the CPU oracle; GameRecord (decoding, events,
moves, rendering against the reference's own text, save / load) and tools/replay.py on the model's buffers.  The GPU suite
(test_gpu_game_record.py) holds the kernel to this model word for word."""
import functools
import importlib.util
import io
import os

import numpy as np
import pytest

import _episode_stats_ref as R
import _game_record_ref as GR
import _golden as G
import _midgame as M
from oracle import oracle as O

TRAJ = G.names("traj_*.npz")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("pos", "dir", "pac", "scared", "carry", "ret", "food", "caps", "score")
UNDETERMINED_SHARE = 0.01                # the issue's bound on move code 7, over all recorded sub-steps


def _game_record():
    from pmx import game_record
    return game_record


def _stats_state(f):
    return R.State(f.pos, f.dir, f.pac, f.scared, f.carry, f.ret, f.caps, f.score)


def _wall(rows, x, y):
    return rows[len(rows) - 1 - y][x] == "%"


def _effective(rows, pos, action):
    """the action the rules apply for a request: itself if it is one of the five and leads to an open cell, else Stop"""
    if action not in GR.VECTORS:
        return 4
    v = GR.VECTORS[action]
    return 4 if _wall(rows, pos[0] + v[0], pos[1] + v[1]) else action


@functools.lru_cache(maxsize=None)
def _fixture_logs(name):
    """one Log per episode of a trajectory fixture (the unfinished tail too) -> (d, meta, [(Log, first tick)])"""
    d, meta = G.load(name)
    H = len(d["init_food"])
    T = len(d["done"])
    logs, log, first = [], GR.Log(GR.fixture_frame(d), H, T), 0
    for t in range(T):
        log.update([GR.fixture_frame(d, t, s) for s in range(4)], d["done"][t])
        if d["done"][t] or t == T - 1:
            logs.append((log, first))
            log, first = GR.Log(GR.fixture_frame(d), H, T), t + 1
    return d, meta, logs


def _record_of(logs, layouts):
    head, frames = GR.buffers(logs)
    return _game_record().GameRecord(head, frames, layouts, dict(source="model"))


def _check_log_against_actions(log, rows, applied, bad, tally):
    """the four EVENT properties of the issue on one Log; applied[k]: the effective action of sub-step k (frame k + 1)"""
    for k in range(1, len(log.frames)):
        X, (Y, ev) = log.frames[k - 1][0], log.frames[k]
        m = (k - 1) % 4
        move, mover_died, victims = ev[0], ev[1], ev[2]
        sx, sy = _stats_state(X), _stats_state(Y)
        if mover_died != R.mover_died(sx, sy, m) or set(victims) != {i for i in range(4) if i != m and R.nonmover_died(sx, sy, i)}:
            bad.append(("deaths", k, ev))
        tally["substeps"] += 1
        if move == 7:
            tally["undetermined"] += 1
            if len(GR.death_candidates(X, m)) == 1 or not mover_died:
                bad.append(("a 7 with one candidate", k, ev))
        elif move != applied[k - 1]:
            bad.append(("move", k, ev, applied[k - 1], X.pos[m], Y.pos[m]))


def test_fixture_list():
    assert len(TRAJ) == 10


@pytest.mark.parametrize("name", TRAJ)
def test_model_on_a_golden_trajectory(name):
    """every frame decodes to the fixture's state after that sub-step; death bits, moves and 7s as the issue states them"""
    d, meta, logs = _fixture_logs(name)
    rows = list(meta["layout"])
    rec = _record_of([l for l, _ in logs], [rows])
    bad, tally = [], dict(substeps=0, undetermined=0)
    for g, (log, first) in enumerate(logs):
        assert rec.length(g) == log.len and rec.done(g) == bool(log.done) and not rec.overflow(g)
        for t in range(log.len):
            for s in range(4):
                got = rec.state(g, t, s)
                for k in FIELDS:
                    want = d["sub_" + k][first + t, s]
                    assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want).astype(np.int64)), (name, g, t, s, k)
        applied = []
        for t in range(log.len):
            for m in range(4):
                X = log.frames[4 * t + m][0]
                applied.append(_effective(rows, X.pos[m], int(d["actions"][first + t, m])))
        _check_log_against_actions(log, rows, applied, bad, tally)
        mv = rec.moves(g)
        assert mv.shape == (log.len, 4) and mv.dtype == np.int8
        assert [(-1 if e[0] == 7 else e[0]) for _, e in log.frames[1:]] == mv.reshape(-1).tolist()
    print(name, tally)
    assert bad == [], (name, len(bad), bad[:5])
    assert tally["undetermined"] < UNDETERMINED_SHARE * tally["substeps"]


def test_undetermined_moves_on_the_oracles_states_alone():
    """The bound on code 7 from the fixtures' states and nothing of the model but the candidate rule: a mover that died (its cell is
    neither its old cell nor old cell + the recorded action) with zero or several enemy cells within one step."""
    sub = und = deaths = 0
    for name in TRAJ:
        d, meta = G.load(name)
        X = GR.fixture_frame(d)
        for t in range(len(d["done"])):
            for m in range(4):
                Y = GR.fixture_frame(d, t, m)
                v = GR.VECTORS.get(int(d["actions"][t, m]), (0, 0))
                gone = Y.pos[m] not in (X.pos[m], (X.pos[m][0] + v[0], X.pos[m][1] + v[1]))
                sub, deaths = sub + 1, deaths + gone
                und += gone and len(GR.death_candidates(X, m)) != 1
                X = Y
            if d["done"][t]:
                X = GR.fixture_frame(d)
    print("sub-steps", sub, "mover deaths", deaths, "undetermined", und)
    assert deaths >= 100 and und < UNDETERMINED_SHARE * sub


@functools.lru_cache(maxsize=None)
def _oracle_logs(board, N=40, T=M.T):
    """N mid-game states of `board` (tests/_midgame.py), each stepped T ticks by a single-env oracle under the mixed action stream
    -> (rows, [Log], [applied actions per log], [the oracle's states per log])"""
    rows = list(M.board_rows(board))
    H = len(rows)
    rng = np.random.RandomState(M.ACTION_SEED)
    logs, applied, states = [], [], []
    for e, p in enumerate(M.start_states(board, N)):
        env = O.Env(rows, length=M.LENGTH)
        env.set_state(p)
        log, app, sts = GR.Log(GR.frame_of(env.get_state(), H), H, T), [], []
        for t in range(T):
            legal = np.array([[env.legal(i) for i in range(4)]], np.uint8)
            out = env.tick(M.mixed_actions(rng, legal, 1)[0])
            if any(out["subout"][i].fault for i in range(4)):
                break
            subs = [GR.frame_of(out["sub"][s], H) for s in range(4)]
            log.update(subs, out["done"])
            app += [int(out["subout"][i].applied_action) for i in range(4)]
            sts += subs
            if out["done"]:
                break
        logs.append(log)
        applied.append(app)
        states.append(sts)
    return rows, logs, applied, states


@pytest.mark.parametrize("board", ("smallCapture", "tinyCapture", "bloxCapture"))
def test_model_on_oracle_stepped_midgame_states(board):
    rows, logs, applied, states = _oracle_logs(board)
    rec = _record_of(logs, [rows])
    bad, tally = [], dict(substeps=0, undetermined=0)
    events = dict(died=0, victims=0, ate=0, capsule=0, returned=0)
    for g, log in enumerate(logs):
        assert len(log.frames) == 1 + len(states[g]) == 1 + 4 * log.len
        for k, want in enumerate(states[g]):
            got = rec.state(g, k // 4, k % 4)
            back = GR.Frame(got["pos"], got["dir"], got["pac"], got["scared"], got["carry"], got["ret"], got["caps"], got["food"], got["score"],
                            len(rows))
            assert back.same_state(want), (board, g, k)
        _check_log_against_actions(log, rows, applied[g], bad, tally)
        for ev in rec.events(g):
            events["died"] += ev[3]
            events["victims"] += len(ev[4])
            events["ate"] += ev[5]
            events["capsule"] += ev[6]
            events["returned"] += ev[7]
    print(board, tally, events)
    assert bad == [], (board, len(bad), bad[:5])
    assert tally["undetermined"] < UNDETERMINED_SHARE * tally["substeps"]
    assert events["died"] > 0 and events["victims"] > 0 and events["ate"] > 0 and events["returned"] > 0
    if board not in M.NO_CAPSULES:
        assert events["capsule"] > 0


def test_score_word_follows_the_returned_pellets():
    """the kernel derives the score after sub-steps 0 .. 2 (the snapshots carry none): previous + / - the mover's returned pellets"""
    for name in TRAJ:
        d, _, logs = _fixture_logs(name)
        for log, _ in logs:
            for k in range(1, len(log.frames)):
                X, (Y, ev) = log.frames[k - 1][0], log.frames[k]
                m = (k - 1) % 4
                assert Y.score == X.score + (ev[5] if m % 2 == 0 else -ev[5]), (name, k)


def test_overflow_and_freeze_in_the_model():
    d, _, _ = _fixture_logs("traj_small_hunter.npz")
    H = len(d["init_food"])
    log = GR.Log(GR.fixture_frame(d), H, 5, fill=-7)
    for t in range(8):
        log.update([GR.fixture_frame(d, t, s) for s in range(4)], 0)
    assert (log.len, log.done, log.overflow) == (5, 0, 1) and len(log.frames) == 21
    assert (log.words()[:21] != -7).any(1).all() and log.words().shape == (21, 12 + H)
    log = GR.Log(GR.fixture_frame(d), H, 20, fill=-7)
    for t in range(8):
        log.update([GR.fixture_frame(d, t, s) for s in range(4)], t == 2)
    assert (log.len, log.done, log.overflow) == (3, 1, 0) and (log.words()[13:] == -7).all()


def test_render_equals_the_references_text():
    gr = _game_record()
    fx = G.load_json("G13_render.json")
    recs = fx["records"]
    assert 30 <= len(recs) <= 45
    pac_dirs, seen = set(), dict(scared=0, caps_eaten=0, red_pac=0, blue_pac=0)
    for r in recs:
        rows = fx["layouts"][r["src"]]
        H = len(rows)
        log = GR.Log(GR.Frame(*(r[k] for k in ("pos", "dir", "pac", "scared", "carry", "ret", "caps", "food", "score")), H), H, 1)
        head, frames = GR.buffers([log])
        rec = gr.GameRecord(head, frames, [rows])
        assert rec.render(0, -1) == r["text"], (r["src"], r["tick"], r["sub"], rec.render(0, -1), r["text"])
        assert rec.render(0, -1).endswith("\nScore: %d\n" % r["score"])
        pac_dirs |= {r["dir"][i] for i in range(4) if r["pac"][i]}
        seen["scared"] += max(r["scared"]) > 0
        seen["caps_eaten"] += sum(bin(c).count("1") for c in r["caps"]) < "".join(rows).count("o")
        seen["red_pac"] += bool(r["pac"][0] or r["pac"][2])
        seen["blue_pac"] += bool(r["pac"][1] or r["pac"][3])
    assert pac_dirs >= {0, 1, 2, 3} and all(v > 0 for v in seen.values()), (pac_dirs, seen)


def _replay_tool():
    spec = importlib.util.spec_from_file_location("pmx_replay_tool", os.path.join(ROOT, "tools", "replay.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_save_load_round_trip_and_replay_tool(tmp_path):
    gr = _game_record()
    d, meta, logs = _fixture_logs("traj_small_hunter.npz")
    rows = list(meta["layout"])
    rec = _record_of([l for l, _ in logs], [rows])
    path = str(tmp_path / "games.npz")
    rec.save(path)
    back = gr.GameRecord.load(path)
    n = 1 + 4 * max(rec.length(g) for g in range(rec.games))
    assert np.array_equal(back.head, rec.head) and np.array_equal(back.frames, rec.frames[:n])
    assert back.layouts == [rows] and back.meta == {"source": "model"} and back.games == len(logs)
    assert back.events(1) == rec.events(1) and back.render(1, 7, 2) == rec.render(1, 7, 2)
    tool = _replay_tool()
    out = io.StringIO()
    assert tool.main([path, "--game", "0", "--from", "3", "--to", "4", "--substeps"], out=out) == 0
    text = out.getvalue()
    assert text.count("Score:") == 8 and rec.render(0, 3, 0) in text and rec.render(0, 4, 3) in text and "tick 3.0" in text
    out = io.StringIO()
    assert tool.main([path, "--events"], out=out) == 0
    lines = out.getvalue().splitlines()
    loud = [e for e in rec.events(0) if e[3] or e[4] or e[5] or e[6] or e[7]]
    assert len(lines) == 1 + len(loud) and len(loud) > 10 and any("dies" in ln for ln in lines) and any("eats a pellet" in ln for ln in lines)
    out = io.StringIO()
    assert tool.main([path, "--to", "1"], out=out) == 0
    assert out.getvalue().count("Score:") == 3 and "start" in out.getvalue()


def test_record_rejects_buffers_of_another_board():
    gr = _game_record()
    with pytest.raises(ValueError):
        gr.GameRecord(np.zeros((8, 2), np.int32), np.zeros((5, 12 + 9, 2), np.int32), [["%" * 6] * 7])
