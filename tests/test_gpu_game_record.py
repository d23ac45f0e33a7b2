"""pmx_game_record_init / pmx_game_record_update against the plain-numpy model tests/_game_record_ref.py (which
tests/test_game_record_cpu.py pins to the golden trajectories and to oracle-stepped states): every word of the head and of every frame
on an offset range with a partial wavefront, mid-game states, raw requests and in-kernel bots, the three plane types, the one-launch
tick's snapshots and a multi-layout handle; the frames against pmx_get_state; freezing and overflow on a sentinel-filled log; the
contract of the entry points; and play_match(record=k)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _game_record_ref as GR
import _midgame as M

pytestmark = pytest.mark.gpu

N, FIRST, COUNT, TICKS = 130, 3, 70, 40
SEED = 11
SENT = -0x5A5A5A5B                        # fills the log before init: a word the kernel never writes
N_MAZES = 48
STATE = np.dtype([("pos", np.int8, (4, 2)), ("dir", np.int8, 4), ("pac", np.uint8, 4), ("scared", np.uint8, 4), ("carry", np.uint16, 4),
                  ("ret", np.uint16, 4), ("food", np.uint32, 32), ("caps", np.uint32, 32), ("score", np.int32), ("steps", np.int32),
                  ("ticks", np.uint32)])


def _frames(env, first, count):
    """the current state of the envs first .. first + count - 1 -> [GR.Frame]"""
    import pmx
    assert STATE.itemsize == C.sizeof(pmx._lib.State)
    return GR.frames_of_records(np.frombuffer(env.get_state(first, count), dtype=STATE), env.layout.height)


@functools.lru_cache(maxsize=None)
def _pool():
    from pmx import maze_generator
    return tuple(maze_generator.generate_maze(k + 1) for k in range(N_MAZES))


def _make(pmx, board, n, dtype, bots, length=300):
    kw = dict(length=length, auto_reset=False, obs_dtype=dtype, seed=SEED, bots=bots)
    if board == "mazes":
        return pmx.PmxVecEnv([pmx.Layout.from_text(t) for t in _pool()], n, layout_index=np.arange(n) % N_MAZES, **kw)
    return pmx.PmxVecEnv(board, n, **kw)


@functools.lru_cache(maxsize=None)
def _start_states(board, n):
    if board == "mazes":                 # every env on its own maze: one drawn mid-game state each
        return tuple(M.random_states(tuple(_pool()[e % N_MAZES].split("\n")), 1, 100 + e)[0] for e in range(n))
    return tuple(M.start_states(board, n))


def _new_record(env, first, count, max_ticks, tail=0):
    """a DeviceGameRecord whose buffers are sentinel-filled, the frames followed by `tail` sentinel words -> (rec, the tail's view)"""
    rec = env.new_game_record(first, count, max_ticks)
    words = rec.frames.numel()
    flat = torch.full((words + tail,), SENT, dtype=torch.int32, device=env.device)
    rec.frames = flat[:words].view(rec.frames.shape)
    rec.head.fill_(SENT)
    return rec, flat[words:]


# (board, plane type, in-kernel baseline bots on the blue side, the one-launch tick)
CASES = [("tinyCapture", "float32", False, False), ("tinyCapture", "uint8", True, False), ("smallCapture", "bfloat16", True, False),
         ("smallCapture", "float32", False, True), ("smallCapture", "uint8", False, False), ("mazes", "bfloat16", False, False)]


@pytest.mark.parametrize("board, dtype, bots, fused", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_every_word_equals_the_model(board, dtype, bots, fused):
    """Two handles with one seed from the same mid-game states: A runs pmx_step + pmx_game_record_update on rows 3 .. 72 of 130, B the
    four pmx_step_agent calls with the same codes and hands its state after every sub-step to the model.  Every head word and every
    frame word, untouched ones included, every ten ticks and at the end; frame 4 t + 4 against A's own pmx_get_state after tick t."""
    import pmx
    n = 128 if fused else N              # the one-launch tick takes whole rule waves only; the range still ends inside a wavefront
    A, B = _make(pmx, board, n, dtype, bots), _make(pmx, board, n, dtype, bots)
    if fused:
        A.set_tuning("fused_min_envs", 64)
    H = A.layout.height
    for env in (A, B):
        env.reset(want_obs=False)
        M.load_states(pmx, env, list(_start_states(board, n)))
    dev = A.device
    rec, _ = _new_record(A, FIRST, COUNT, TICKS)
    assert rec.frame_words == 12 + H and rec.frames.shape == (1 + 4 * TICKS, 12 + H, COUNT)
    A.game_record_init(rec)
    layout_of = (lambda e: e % N_MAZES) if board == "mazes" else (lambda e: 0)
    logs = [GR.Log(f, H, TICKS, layout=layout_of(FIRST + r), fill=SENT) for r, f in enumerate(_frames(B, FIRST, COUNT))]

    def compare(t):
        head, frames = GR.buffers(logs)
        got_h, got_f = rec.head.cpu().numpy(), rec.frames.cpu().numpy()
        assert (got_h == head).all(), (board, t, np.nonzero((got_h != head).any(0))[0][:8])
        bad = np.argwhere(got_f != frames)
        assert len(bad) == 0, (board, t, len(bad), bad[:4], [(got_f[tuple(b)], frames[tuple(b)]) for b in bad[:4]])

    compare(-1)
    gen = torch.Generator(device="cpu").manual_seed(SEED)
    after_tick = []
    for t in range(TICKS):
        acts = torch.randint(0, 5, (n, 4), generator=gen).to(torch.int8)          # uniform requests: about a third illegal
        if bots:
            acts[:, 1], acts[:, 3] = -3, -4                                        # baselineTeam plays blue inside the kernel
        acts = acts.to(dev)
        A.step(acts, want_obs=True)
        assert A.last_step_fused() == fused
        subs = []
        for agent in range(4):
            B.step_agent(agent, acts[:, agent].contiguous(), want_obs=False)
            subs.append(_frames(B, FIRST, COUNT))
        assert torch.equal(A.done, B.done)
        done = A.done.cpu().numpy()
        for r, log in enumerate(logs):
            log.update([subs[m][r] for m in range(4)], done[FIRST + r])
        A.game_record_update(rec, A.done)
        after_tick.append(_frames(A, FIRST, COUNT))
        if t % 10 == 9:
            compare(t)
    compare(TICKS)
    host = rec.to_host()
    tally = dict(died=0, victims=0, ate=0, returned=0, undetermined=0, done=0)
    for g in range(COUNT):
        assert host.length(g) == logs[g].len and host.done(g) == bool(logs[g].done) and not host.overflow(g)
        tally["done"] += host.done(g)
        for t in range(host.length(g)):
            s = host.state(g, t, 3)
            back = GR.Frame(s["pos"], s["dir"], s["pac"], s["scared"], s["carry"], s["ret"], s["caps"], s["food"], s["score"], H)
            assert back.same_state(after_tick[t][g]), (board, g, t)
        for ev in host.events(g):
            tally["died"] += ev[3]
            tally["victims"] += len(ev[4])
            tally["ate"] += ev[5]
            tally["returned"] += ev[7]
            tally["undetermined"] += ev[2] == -1
    print(board, dtype, bots, tally)
    assert tally["ate"] > 0 and tally["returned"] > 0 and tally["died"] + tally["victims"] > 0
    if board == "mazes":
        assert sorted(set(host.head[3].tolist())) == sorted({(FIRST + r) % N_MAZES for r in range(COUNT)})
        assert host.render(0, 0).count("\n") == H + 1
    A.close()
    B.close()


def _bot_run(pmx, n, length):
    env = pmx.PmxVecEnv("smallCapture", n, length=length, auto_reset=False, obs_dtype="uint8", seed=SEED, bots=True)
    env.reset(want_obs=False)
    return env, torch.tensor((-3, -3, -4, -4), dtype=torch.int8, device=env.device)[None].expand(n, 4).contiguous()


def test_a_done_row_freezes():
    """length = 12, max_ticks = 20: every game is done after 13 ticks; four more steps and updates change no word of the log"""
    import pmx
    env, acts = _bot_run(pmx, N, 12)
    rec, tail = _new_record(env, FIRST, COUNT, 20, tail=1024)
    env.game_record_init(rec)
    for t in range(13):
        env.step(acts, want_obs=False)
        env.game_record_update(rec, env.done)
    head, frames = rec.head.clone(), rec.frames.clone()
    assert (head[0] == 13).all() and (head[1] == 1).all() and (head[2] == 0).all() and (head[3:] == 0).all()
    assert (frames[:53] != SENT).all() and (frames[53:] == SENT).all()
    for t in range(4):
        env.step(acts, want_obs=False)
        env.game_record_update(rec, env.done)
    assert torch.equal(rec.head, head) and torch.equal(rec.frames, frames) and (tail == SENT).all()
    env.close()


def test_a_full_log_sets_overflow_and_writes_nothing_more():
    """max_ticks = 5: LEN stays 5, OVERFLOW is set by the sixth update, nothing past frame 20 is touched"""
    import pmx
    env, acts = _bot_run(pmx, N, 300)
    rec, tail = _new_record(env, FIRST, COUNT, 5, tail=4096)
    env.game_record_init(rec)
    for t in range(5):
        env.step(acts, want_obs=False)
        env.game_record_update(rec, env.done)
    assert (rec.head[0] == 5).all() and (rec.head[2] == 0).all()
    frames = rec.frames.clone()
    assert (frames != SENT).all()
    for t in range(3):
        env.step(acts, want_obs=False)
        env.game_record_update(rec, env.done)
        assert (rec.head[0] == 5).all() and (rec.head[1] == 0).all() and (rec.head[2] == 1).all() and (rec.head[3:] == 0).all()
    assert torch.equal(rec.frames, frames) and (tail == SENT).all()
    host = rec.to_host()
    assert all(host.overflow(g) and host.length(g) == 5 for g in range(COUNT)) and host.frames.shape[0] == 21
    env.close()


def test_contract():
    import pmx
    L = pmx._lib
    n = 131
    env, acts = _bot_run(pmx, n, 300)
    twin, _ = _bot_run(pmx, n, 300)
    dev = env.device
    st = L.stream(dev)
    call = lambda name, *a: getattr(env.lib, name)(env.handle, *a, st)
    INVALID, UNSUPPORTED = -1, -2
    fw = C.c_int32()
    assert env.lib.pmx_game_record_words(env.handle, C.byref(fw)) == 0 and fw.value == 12 + env.layout.height
    assert env.lib.pmx_game_record_words(None, C.byref(fw)) == INVALID and env.lib.pmx_game_record_words(env.handle, None) == INVALID
    rec, tail = _new_record(env, 0, n, 8, tail=1024)
    env.game_record_init(rec)
    h, f = rec.head.data_ptr(), rec.frames.data_ptr()
    # a handle that records leaves the same stats rows and the same outputs as a twin that does not; an open profile counts the update
    s_env, s_twin = env.episode_stats_init(env.new_episode_stats()), twin.episode_stats_init(twin.new_episode_stats())
    launches = []
    for t in range(6):
        for e, recorded in ((env, True), (twin, False)):
            e.profile_begin(8)
            e.step(acts, want_obs=False)
            e.episode_stats_update(s_env if recorded else s_twin, e.done)
            if recorded:
                e.game_record_update(rec, e.done)
            launches.append(e.profile_end()["rule_launches"])
        assert launches[-2] == launches[-1] + 1
        for k in ("reward", "done", "legal", "score", "agent"):
            assert torch.equal(getattr(env, k), getattr(twin, k)), (t, k)
        assert torch.equal(s_env, s_twin)
    assert bytes(env.get_state()) == bytes(twin.get_state())
    assert (rec.head[0] == 6).all() and (tail == SENT).all()
    head, frames = rec.head.clone(), rec.frames.clone()
    # count == 0 launches nothing and is no error, at either end of the handle
    assert call("pmx_game_record_init", 0, 0, 8, h, f) == 0 and call("pmx_game_record_update", n, 0, 8, None, h, f) == 0
    # errors
    assert env.lib.pmx_game_record_init(None, 0, 1, 8, h, f, st) == INVALID and env.lib.pmx_game_record_update(None, 0, 1, 8, None, h, f, st) == INVALID
    assert call("pmx_game_record_init", 0, 1, 8, None, f) == INVALID and call("pmx_game_record_init", 0, 1, 8, h, None) == INVALID
    assert call("pmx_game_record_update", 0, 1, 8, None, None, f) == INVALID and call("pmx_game_record_update", 0, 1, 8, None, h, None) == INVALID
    for fi, c in ((-1, 1), (0, -1), (n, 1), (1, n), (2 ** 31 - 1, 2)):
        assert call("pmx_game_record_init", fi, c, 8, h, f) == INVALID, (fi, c)
        assert call("pmx_game_record_update", fi, c, 8, None, h, f) == INVALID, (fi, c)
    for mt in (0, -1):
        assert call("pmx_game_record_init", 0, n, mt, h, f) == INVALID and call("pmx_game_record_update", 0, n, mt, None, h, f) == INVALID
        assert b"max_ticks" in env.lib.pmx_last_error()
    env.reset(want_obs=False)                                    # nothing stepped since: the snapshots describe no tick
    assert call("pmx_game_record_update", 0, n, 8, None, h, f) == INVALID
    assert b"snapshots" in env.lib.pmx_last_error()
    env.step(acts, want_obs=False)
    env.set_state(env.get_state(0, 1))
    assert call("pmx_game_record_update", 0, n, 8, None, h, f) == INVALID
    env.step(acts, want_obs=False)
    env.step_agent(0, acts[:, 0].contiguous(), want_obs=False)    # an open tick
    assert call("pmx_game_record_update", 0, n, 8, None, h, f) == INVALID and call("pmx_game_record_init", 0, n, 8, h, f) == INVALID
    assert torch.equal(rec.head, head) and torch.equal(rec.frames, frames) and (tail == SENT).all()
    env.close()
    twin.close()
    auto = pmx.PmxVecEnv("smallCapture", 64, length=300, auto_reset=True, obs_dtype="uint8", seed=SEED)
    auto.reset(want_obs=False)
    buf = auto.new_game_record()
    with pytest.raises(L.PmxError, match="code -2"):
        auto.game_record_init(buf)
    auto.step(torch.full((64, 4), 4, dtype=torch.int8, device=dev), want_obs=False)
    assert auto.lib.pmx_game_record_update(auto.handle, 0, 64, buf.max_ticks, None, buf.head.data_ptr(), buf.frames.data_ptr(), st) == UNSUPPORTED
    assert (buf.head == 0).all() and (buf.frames == 0).all()
    auto.close()


def test_play_match_records_the_first_games(monkeypatch):
    import pmx
    from pmx import trainer
    calls = []
    real = pmx._lib.call
    monkeypatch.setattr(pmx._lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    kw = dict(layout="tinyCapture", n_envs=64, length=60, seed=5)
    sides = lambda: (trainer.MatchSide(bot="baseline"), trainer.MatchSide(bot="random"))
    r0 = trainer.play_match(*sides(), **kw)
    assert r0["record"] is None and not [c for c in calls if "game_record" in c] and "pmx_episode_stats_update" in calls
    r = trainer.play_match(*sides(), record=3, **kw)
    rec = r["record"]
    assert calls.count("pmx_game_record_init") == 1 and calls.count("pmx_game_record_update") == calls.count("pmx_episode_stats_update") // 2
    assert rec.games == 3 and torch.equal(r["score"], r0["score"]) and torch.equal(r["stats"], r0["stats"])
    for g in range(3):
        assert rec.done(g) and not rec.overflow(g)
        assert rec.final_score(g) == int(r["score"][g]) and rec.length(g) == int(r["stats"][pmx._lib.STATS_W_TICKS, g])
    assert rec.meta["a_is_red"] == r["red"][:3].tolist() and rec.meta["side_a"] == "baseline" and rec.meta["length"] == 60
    assert trainer.play_match(*sides(), record=1000, **kw)["record"].games == 64          # clipped to n_envs
