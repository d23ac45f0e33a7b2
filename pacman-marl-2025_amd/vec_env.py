"""PmxVecEnv: N independent Capture-the-Flag games advanced in lock-step by the HIP kernels.

Tensor-level mirror of gymPacMan.gymPacMan_parallel_env (gymPacMan.py:15-270): same constructor meaning, same
step()/reset() results, but every result carries a leading env dimension and lives on the GPU.  PyTorch is used
only for device memory and the current stream; all compute is in libpmx_hip.so through the C ABI.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .layout import Layout, get_layout

_DTYPES = {"float32": (_lib.OBS_F32, torch.float32), "bfloat16": (_lib.OBS_BF16, torch.bfloat16),
           "uint8": (_lib.OBS_U8, torch.uint8)}
# reference order of a legal-action list: N, S, E, W, Stop as ints 0,2,1,3,4 (game.py:295-299, gymPacMan.py:78-89)
LEGAL_LIST_ORDER = (0, 2, 1, 3, 4)


def legal_list(mask):
    return [a for a in LEGAL_LIST_ORDER if (int(mask) >> a) & 1]


class DeviceGameRecord:
    """The two caller-owned buffers of include/pmx.h, "Game records", for `count` envs from `first`: head int32 [8, count] and
    frames int32 [1 + 4 max_ticks, frame_words, count], zeroed (PmxVecEnv.new_game_record)."""

    def __init__(self, env, first, count, max_ticks, frame_words):
        self.env, self.first, self.count, self.max_ticks, self.frame_words = env, first, count, max_ticks, frame_words
        self.head = torch.zeros((_lib.RECORD_HEAD_WORDS, count), dtype=torch.int32, device=env.device)
        self.frames = torch.zeros((1 + 4 * max_ticks, frame_words, count), dtype=torch.int32, device=env.device)

    def to_host(self, **meta):
        """-> game_record.GameRecord: the head, the frames up to the longest game, the env's layouts and the metadata (one
        device-to-host copy of each buffer; synchronises)."""
        from .game_record import GameRecord
        head = self.head.cpu().numpy()
        n = 1 + 4 * min(self.max_ticks, max(0, int(head[_lib.RECORD_LEN].max(initial=0))))
        meta = dict(dict(first=self.first, max_ticks=self.max_ticks, length=self.env.length), **meta)
        return GameRecord(head, self.frames[:n].cpu().numpy(), [list(l.text) for l in self.env.layouts], meta)


class PmxVecEnv:
    def __init__(self, layout, n_envs, length=299, reward_forLegalAction=True, defenceReward=True, auto_reset=True,
                 obs_dtype="float32", obs_agents=(0, 1, 2, 3), device="cuda:0", seed=0, layout_index=None, bots=False,
                 redraw_layouts=False):
        if not torch.cuda.is_available():
            raise _lib.PmxError("PmxVecEnv needs a GPU: the product has no CPU path")
        self.lib = _lib.load()
        # `layout` may be one layout (name / Layout) or a list of equally sized Layouts with `layout_index` [n_envs]
        layouts = None
        if isinstance(layout, (list, tuple)):
            layouts = list(layout)
            layout = layouts[0]
        if isinstance(layout, str):
            lay = get_layout(layout)
            if lay is None:
                raise FileNotFoundError(layout)
            layout = lay
        assert isinstance(layout, Layout)
        self.layout = layout
        self.layouts = layouts if layouts is not None else [layout]
        if any((l.width, l.height) != (layout.width, layout.height) for l in self.layouts):
            raise ValueError("all layouts of one PmxVecEnv must have the same width and height")
        self.n_envs = int(n_envs)
        self.length = int(length)
        self.device = torch.device(device)
        self.obs_code, self.obs_torch_dtype = _DTYPES[obs_dtype]
        self.obs_agents = tuple(sorted(set(int(a) for a in obs_agents)))
        cfg = _lib.Config()
        cfg.width, cfg.height = layout.width, layout.height
        L = self.layouts
        self._keep = (np.ascontiguousarray(np.stack([l.wall_rows for l in L])), np.ascontiguousarray(np.stack([l.food_rows for l in L])),
                      np.ascontiguousarray(np.stack([l.cap_rows for l in L])), np.ascontiguousarray(np.stack([l.starts for l in L])))
        if len(L) > 1:
            if layout_index is None:
                layout_index = np.arange(int(n_envs)) % len(L)
            self.layout_index = np.ascontiguousarray(layout_index, np.int32)
            assert self.layout_index.shape == (int(n_envs),)
            cfg.n_layouts = len(L)
            cfg.layout_index = self.layout_index.ctypes.data_as(C.POINTER(C.c_int32))
        else:
            self.layout_index = None
        cfg.wall_rows = self._keep[0].ctypes.data_as(C.POINTER(C.c_uint32))
        cfg.food_rows = self._keep[1].ctypes.data_as(C.POINTER(C.c_uint32))
        cfg.cap_rows = self._keep[2].ctypes.data_as(C.POINTER(C.c_uint32))
        cfg.starts = self._keep[3].ctypes.data_as(C.POINTER(C.c_int8))
        cfg.n_envs, cfg.length = self.n_envs, self.length
        cfg.legal_reward, cfg.defence_reward = int(bool(reward_forLegalAction)), int(bool(defenceReward))
        cfg.auto_reset = int(bool(auto_reset))
        cfg.obs_dtype = self.obs_code
        cfg.obs_agents = sum(1 << a for a in self.obs_agents)
        cfg.device = self.device.index or 0
        cfg.seed = int(seed) & 0xFFFFFFFF
        # random_layout=True of the reference (gymPacMan.py:98-100): an env moves to a freshly drawn layout of the pool at every
        # reset; `layout` is then the pool of generated mazes
        cfg.redraw_layouts = int(bool(redraw_layouts))
        if redraw_layouts and len(L) < 2:
            raise ValueError("redraw_layouts needs a pool of at least two layouts")
        cfg.enable_bots = int(bool(bots))          # understand ACTION_BASELINE_* / ACTION_APPROXQ_* (in-kernel bot teams)
        self.handle = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.call("pmx_create", C.byref(cfg), C.byref(self.handle))
        N, H, W = self.n_envs, layout.height, layout.width
        self.n_emit = len(self.obs_agents)
        self.obs_shape = (8, H, W)
        dev = self.device
        self.obs = torch.empty((N, self.n_emit, 8, H, W), dtype=self.obs_torch_dtype, device=dev)
        self.reward = torch.empty((N, 2), dtype=torch.float64, device=dev)
        self.done = torch.empty((N,), dtype=torch.uint8, device=dev)
        self.legal = torch.empty((N, 4), dtype=torch.uint8, device=dev)
        self.score_change = torch.empty((N,), dtype=torch.int32, device=dev)
        self.score = torch.empty((N,), dtype=torch.int32, device=dev)
        self.agent = torch.zeros((N, 4), dtype=torch.int32, device=dev)   # x | y<<8 | carry<<16 after own sub-step
        self._agent_obs = None

    # -- plumbing -------------------------------------------------------------------------------------------------
    def _out(self, obs=True, obs_tensor=None):
        o = _lib.StepOut()
        t = obs_tensor if obs_tensor is not None else self.obs
        o.obs_dev = t.data_ptr() if obs else None
        o.reward_dev = self.reward.data_ptr()
        o.done_dev = self.done.data_ptr()
        o.legal_dev = self.legal.data_ptr()
        o.score_change_dev = self.score_change.data_ptr()
        o.score_dev = self.score.data_ptr()
        o.agent_dev = self.agent.data_ptr()
        return o

    def close(self):
        if getattr(self, "handle", None) and self.handle.value:
            self.lib.pmx_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- gymPacMan surface, batched -----------------------------------------------------------------------------
    def reset(self, mask=None, want_obs=True):
        """gymPacMan.reset (gymPacMan.py:92-141).  mask: uint8/bool [N] tensor of envs to reset, None = all.
        Returns (obs [N,n_emit,8,H,W], legal [N,4] bit masks)."""
        m = None
        if mask is not None:
            m = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            assert m.shape == (self.n_envs,)
        out = self._out(obs=want_obs)
        with torch.cuda.device(self.device):
            _lib.call("pmx_reset", self.handle, m.data_ptr() if m is not None else None, C.byref(out), _lib.stream(self.device))
        return self.obs, self.legal

    def step(self, actions, want_obs=True):
        """gymPacMan.step (gymPacMan.py:143-193) for all envs.  actions: int8 [N,4] (0 N, 1 E, 2 S, 3 W, 4 Stop).
        Returns (obs, reward [N,2] f64 (red, blue), done [N] u8, info dict of tensors).  The returned tensors are
        the env's own output buffers and are overwritten by the next call."""
        a = actions
        if a.dtype != torch.int8 or not a.is_contiguous() or a.device != self.device:
            a = a.to(device=self.device, dtype=torch.int8).contiguous()
        assert a.shape == (self.n_envs, 4)
        out = self._out(obs=want_obs)
        with torch.cuda.device(self.device):
            _lib.call("pmx_step", self.handle, a.data_ptr(), C.byref(out), _lib.stream(self.device))
        return self.obs, self.reward, self.done, {"legal_actions": self.legal, "score_change": self.score_change,
                                                   "score": self.score, "agent": self.agent}

    def step_agent(self, agent, actions, want_obs=True):
        """One agent's sub-step (loop body gymPacMan.py:149-169); agent 3 closes the tick.  actions int8 [N].
        Returns that agent's observation [N,8,H,W] (or None)."""
        a = actions.to(device=self.device, dtype=torch.int8).contiguous()
        assert a.shape == (self.n_envs,)
        if self._agent_obs is None:
            self._agent_obs = torch.empty((4, self.n_envs) + self.obs_shape, dtype=self.obs_torch_dtype, device=self.device)
        out = self._out(obs=want_obs, obs_tensor=self._agent_obs[agent])
        with torch.cuda.device(self.device):
            _lib.call("pmx_step_agent", self.handle, int(agent), a.data_ptr(), C.byref(out), _lib.stream(self.device))
        return self._agent_obs[agent] if want_obs else None

    def successor(self, agent, actions):
        """GameState.generateSuccessor (capture.py:107-123) in place on every env; returns scoreChange [N] int32."""
        a = actions.to(device=self.device, dtype=torch.int8).contiguous()
        assert a.shape == (self.n_envs,)
        with torch.cuda.device(self.device):
            _lib.call("pmx_successor", self.handle, int(agent), a.data_ptr(), self.score_change.data_ptr(), _lib.stream(self.device))
        return self.score_change

    def bot_query(self, agent, code, want_values=True):
        """Ask an in-kernel bot for its move (pmx_bot_query): for `agent` of every env, on the current state and without
        changing it, what bot `code` (-2 .. -6) would play if step_agent(agent, code) were called now.  Returns (values [N,5]
        float64 indexed by action code, NaN where illegal -- None unless want_values --, action [N] int8, flags [N] uint8:
        bit 0 walked home, bit 1 explored; after set_bot_sight also bit 2 / bit 3: the enemy with the lower / higher index is
        seen); fresh tensors."""
        N = self.n_envs
        values = torch.empty((N, 5), dtype=torch.float64, device=self.device) if want_values else None
        action = torch.empty((N,), dtype=torch.int8, device=self.device)
        flags = torch.empty((N,), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.call("pmx_bot_query", self.handle, int(agent), int(code), values.data_ptr() if want_values else None, action.data_ptr(),
                      flags.data_ptr(), _lib.stream(self.device))
        return values, action, flags

    def set_bot_sight(self, sight_range=None):
        """Bind the in-kernel bots (codes -3 .. -6) to the contest's sight rule (pmx_set_bot_sight): a bot then counts an enemy
        only within `sight_range` (1 .. 64) Manhattan cells of itself or its mate, as the reference's bots do under
        GameState.makeObservation.  None switches the rule off (the default).  Applies to every step, step_agent and bot_query
        after the call; needs an env created with bots=True."""
        _lib.call("pmx_set_bot_sight", self.handle, _lib.BOT_SIGHT_OFF if sight_range is None else int(sight_range))

    def set_obs_sight(self, sight_range=None):
        """Put the four-agent observations under the contest's sight rule (pmx_set_obs_sight; GameState.makeObservation,
        capture.py:268-292): in every observation step(), step_agent(), observe() and reset() write after the call, agent i's
        plane 5 shows an enemy only within `sight_range` (0 .. 64) Manhattan cells of i or of its mate, positions from the snapshot
        i's planes are encoded from.  Every other plane and every other output is unchanged.  None switches the rule off (the
        default): the calls are then the ones of an env never set."""
        _lib.call("pmx_set_obs_sight", self.handle, _lib.OBS_SIGHT_OFF if sight_range is None else int(sight_range))

    def agent_distances(self, agent=None, out=None):
        """The contest's getAgentDistances() for every env (pmx_agent_distances; capture.py:210-224): Manhattan distance plus a
        noise of -6 .. 6 from the env's counter-based generator, the draw belief_update makes for the enemies.  agent None: int8
        [N, 4, 4], r[a, i] = agent a's reading of agent i (itself and its mate included) on the state a's planes come from -- its
        sub-step snapshot after step(), the current state otherwise.  agent 0 .. 3: int8 [N, 4], that agent's readings on the
        current state (after step_agent(agent), observe() or reset()).  out: a tensor of that shape to write into; else a fresh
        one.  Changes nothing in the env."""
        if agent is not None and not 0 <= int(agent) <= 3:           # (-1 is the C ABI's code for the [N, 4, 4] form: a larger buffer)
            raise ValueError(f"agent must be None or 0 .. 3, got {agent!r}")
        shape = (self.n_envs, 4, 4) if agent is None else (self.n_envs, 4)
        if out is None:
            out = torch.empty(shape, dtype=torch.int8, device=self.device)
        assert out.shape == shape and out.dtype == torch.int8 and out.is_contiguous() and out.device == self.device
        with torch.cuda.device(self.device):
            _lib.call("pmx_agent_distances", self.handle, -1 if agent is None else int(agent), out.data_ptr(), _lib.stream(self.device))
        return out

    def observe(self, want_obs=True, want_legal=True):
        """get_Observation of the current state for every emitted agent (gymPacMan.py:195-229) and/or the legal masks."""
        with torch.cuda.device(self.device):
            _lib.call("pmx_observe", self.handle, self.obs.data_ptr() if want_obs else None, self.legal.data_ptr() if want_legal else None,
                      _lib.stream(self.device))
        return self.obs, self.legal

    def emit_team_obs(self, team_red, team_obs, merged=None, sight_range=None, belief=None, levels=None):
        """The two observations of one team for the CURRENT tick (canonicalised for red) into team_obs [N,2,8,H,W] and, if
        given, the merged critic input into merged [N,8,H,W] (pmx_emit_team_obs; pacman_mappo_resnet.py:215-229, :267-274).
        sight_range (an int): the contest's fog of war on the two learners' planes (pmx_emit_team_obs_fog; capture.py:268-292),
        an enemy shows only within that Manhattan distance of one of the team's agents; merged stays full-information.
        belief (a new_belief() tensor, in place of sight_range): plane 5 of slot j is the OR of the tracker's two sets of that
        slot (pmx_emit_team_obs_belief); the tensor is only read.
        levels (the levels tensor of new_belief_weights(), in place of both): plane 5 of slot j is levels[:, j] as numbers 0 .. 16
        (pmx_emit_team_obs_weighted); only read."""
        N = self.n_envs
        assert team_obs.shape == (N, 2) + self.obs_shape and team_obs.dtype == self.obs_torch_dtype and team_obs.is_contiguous()
        if merged is not None:
            assert merged.shape == (N,) + self.obs_shape and merged.dtype == self.obs_torch_dtype and merged.is_contiguous()
        with torch.cuda.device(self.device):
            if levels is not None:
                assert sight_range is None and belief is None, "the weighted emission replaces the fog and the belief emission: pass one of the three"
                self._check_levels(levels, N)
                _lib.call("pmx_emit_team_obs_weighted", self.handle, int(bool(team_red)), levels.data_ptr(), team_obs.data_ptr(),
                          merged.data_ptr() if merged is not None else None, _lib.stream(self.device))
                return team_obs, merged
            if belief is not None:
                assert sight_range is None, "the belief emission applies no sight rule of its own: pass one of the two"
                self._check_belief(belief, N)
                _lib.call("pmx_emit_team_obs_belief", self.handle, int(bool(team_red)), belief.data_ptr(), team_obs.data_ptr(),
                          merged.data_ptr() if merged is not None else None, _lib.stream(self.device))
                return team_obs, merged
            if sight_range is not None:
                _lib.call("pmx_emit_team_obs_fog", self.handle, int(bool(team_red)), int(sight_range), team_obs.data_ptr(),
                          merged.data_ptr() if merged is not None else None, _lib.stream(self.device))
                return team_obs, merged
            _lib.call("pmx_emit_team_obs", self.handle, int(bool(team_red)), team_obs.data_ptr(),
                      merged.data_ptr() if merged is not None else None, _lib.stream(self.device))
        return team_obs, merged

    def emit_team_obs_mixed(self, team_red, team_obs, merged=None, first=0, count=None, sight_range=None, belief=None, levels=None):
        """emit_team_obs with the learners' colour chosen per env (pmx_emit_team_obs_mixed): team_red uint8 [N], non-zero = that
        env's learners are red.  Writes rows for the envs first .. first + count - 1 (count None: up to the last env), row j for
        env first + j, into team_obs [count,2,8,H,W] and, if given, merged [count,8,H,W].  sight_range as in emit_team_obs
        (pmx_emit_team_obs_mixed_fog); belief as there too, a [count,2,2,32] tensor whose row j belongs to env first + j
        (pmx_emit_team_obs_mixed_belief); levels likewise, [count,2,HW] (pmx_emit_team_obs_mixed_weighted)."""
        N = self.n_envs
        first = int(first)
        count = N - first if count is None else int(count)
        assert team_red.shape == (N,) and team_red.dtype == torch.uint8 and team_red.is_contiguous() and team_red.device == team_obs.device
        assert team_obs.shape == (count, 2) + self.obs_shape and team_obs.dtype == self.obs_torch_dtype and team_obs.is_contiguous()
        if merged is not None:
            assert merged.shape == (count,) + self.obs_shape and merged.dtype == self.obs_torch_dtype and merged.is_contiguous()
        if count == 0:                                   # (an empty tensor has no address to pass)
            return team_obs, merged
        with torch.cuda.device(self.device):
            if levels is not None:
                assert sight_range is None and belief is None, "the weighted emission replaces the fog and the belief emission: pass one of the three"
                self._check_levels(levels, count)
                _lib.call("pmx_emit_team_obs_mixed_weighted", self.handle, team_red.data_ptr(), first, count, levels.data_ptr(),
                          team_obs.data_ptr(), merged.data_ptr() if merged is not None else None, _lib.stream(self.device))
                return team_obs, merged
            if belief is not None:
                assert sight_range is None, "the belief emission applies no sight rule of its own: pass one of the two"
                self._check_belief(belief, count)
                _lib.call("pmx_emit_team_obs_mixed_belief", self.handle, team_red.data_ptr(), first, count, belief.data_ptr(),
                          team_obs.data_ptr(), merged.data_ptr() if merged is not None else None, _lib.stream(self.device))
                return team_obs, merged
            if sight_range is not None:
                _lib.call("pmx_emit_team_obs_mixed_fog", self.handle, team_red.data_ptr(), first, count, int(sight_range),
                          team_obs.data_ptr(), merged.data_ptr() if merged is not None else None, _lib.stream(self.device))
                return team_obs, merged
            _lib.call("pmx_emit_team_obs_mixed", self.handle, team_red.data_ptr(), first, count, team_obs.data_ptr(),
                      merged.data_ptr() if merged is not None else None, _lib.stream(self.device))
        return team_obs, merged

    # -- belief sets of the hidden enemies (include/pmx.h, "Belief sets") -------------------------------------------
    def new_belief(self, count=None):
        """A belief buffer for `count` envs (None: all): int32 [count, 2 slots, 2 enemies, 32 row words], zeroed; bit x of word y
        = the enemy can be on cell (x, y).  Call belief_init before the first use."""
        return torch.zeros((self.n_envs if count is None else int(count), 2, 2, 32), dtype=torch.int32, device=self.device)

    def _check_belief(self, belief, count):
        assert belief.shape == (count, 2, 2, 32) and belief.dtype == torch.int32 and belief.is_contiguous() and belief.device == self.device

    def belief_init(self, belief, kind=0, first=0, count=None):
        """pmx_belief_init on rows 0 .. count - 1 of `belief` for the envs first .. first + count - 1: kind 0 = the start cells
        (after reset()), kind 1 = every open cell (after set_state(), or when the learners' colour changes)."""
        first = int(first)
        count = self.n_envs - first if count is None else int(count)
        if count == 0:
            return belief
        self._check_belief(belief, count)
        with torch.cuda.device(self.device):
            _lib.call("pmx_belief_init", self.handle, first, count, int(kind), belief.data_ptr(), _lib.stream(self.device))
        return belief

    def belief_update(self, team_red, belief, sight_range, reset=None, first=0, count=None, sonar=None, evidence=None, rules=7):
        """pmx_belief_update, once after each step(): advances the sets of the envs first .. first + count - 1 (row j of `belief`
        for env first + j) by the enemy's motion, the respawn rule, the sight rule and this tick's sonar readings.  team_red: a
        bool, or a uint8 [N] tensor (per env).  reset: uint8 [N], non-zero = that env was reset (pass step()'s done under
        auto_reset): its sets go back to the start cells.  sonar: optional int8 [count, 2, 2] output of the readings.
        evidence (a new_belief_evidence() tensor of `count` rows): pmx_belief_update_evidence instead, with the rule bits `rules`
        (_lib.EVIDENCE_SIDE | EVIDENCE_FOOD | EVIDENCE_CONTACT); None makes the call made before."""
        first = int(first)
        count = self.n_envs - first if count is None else int(count)
        if count == 0:
            return belief
        self._check_belief(belief, count)
        red_dev = None
        if isinstance(team_red, torch.Tensor):
            assert team_red.shape == (self.n_envs,) and team_red.dtype == torch.uint8 and team_red.is_contiguous() and team_red.device == self.device
            red_dev, team_red = team_red.data_ptr(), 0
        if reset is not None:
            assert reset.shape == (self.n_envs,) and reset.dtype == torch.uint8 and reset.is_contiguous() and reset.device == self.device
        if sonar is not None:
            assert sonar.shape == (count, 2, 2) and sonar.dtype == torch.int8 and sonar.is_contiguous() and sonar.device == self.device
        with torch.cuda.device(self.device):
            if evidence is not None:
                self._check_evidence(evidence, count)
                _lib.call("pmx_belief_update_evidence", self.handle, int(bool(team_red)), red_dev, first, count, int(sight_range), int(rules),
                          reset.data_ptr() if reset is not None else None, belief.data_ptr(), sonar.data_ptr() if sonar is not None else None,
                          evidence.data_ptr(), _lib.stream(self.device))
                return belief
            _lib.call("pmx_belief_update", self.handle, int(bool(team_red)), red_dev, first, count, int(sight_range),
                      reset.data_ptr() if reset is not None else None, belief.data_ptr(), sonar.data_ptr() if sonar is not None else None,
                      _lib.stream(self.device))
        return belief

    # -- belief weights: the exact filter that refines the sets (include/pmx.h, "Belief weights") ---------------------
    def new_belief_weights(self, count=None):
        """(weights, levels) for `count` envs (None: all), zeroed: weights int16 [count, 2 slots, 2 enemies, H * W] holding the
        kernel's uint16 values bit for bit (torch has no uint16 in this binding, as belief is int32), levels uint8 [count, 2, H * W].
        Cell y * W + x, raw coordinates.  Call belief_weights_init before the first use."""
        n, hw = self.n_envs if count is None else int(count), self.layout.height * self.layout.width
        return (torch.zeros((n, 2, 2, hw), dtype=torch.int16, device=self.device), torch.zeros((n, 2, hw), dtype=torch.uint8, device=self.device))

    def _check_levels(self, levels, count):
        hw = self.layout.height * self.layout.width
        assert levels.shape == (count, 2, hw) and levels.dtype == torch.uint8 and levels.is_contiguous() and levels.device == self.device

    def _check_weights(self, weights, count):
        hw = self.layout.height * self.layout.width
        assert weights.shape == (count, 2, 2, hw) and weights.dtype == torch.int16 and weights.is_contiguous() and weights.device == self.device

    def belief_weights_init(self, belief, weights, levels, kind=0, first=0, count=None):
        """pmx_belief_weights_init: belief_init on `belief`, the weights 65535 on the cells of each set and the levels to match."""
        first = int(first)
        count = self.n_envs - first if count is None else int(count)
        if count == 0:
            return belief, weights, levels
        self._check_belief(belief, count)
        self._check_weights(weights, count)
        self._check_levels(levels, count)
        with torch.cuda.device(self.device):
            _lib.call("pmx_belief_weights_init", self.handle, first, count, int(kind), belief.data_ptr(), weights.data_ptr(), levels.data_ptr(),
                      _lib.stream(self.device))
        return belief, weights, levels

    def belief_weights_update(self, team_red, belief, weights, levels, sight_range, reset=None, first=0, count=None, sonar=None,
                              evidence=None, rules=7):
        """pmx_belief_weights_update, once after each step() IN PLACE OF belief_update: advances the sets exactly as belief_update
        does and, beside them, the weights (random-walk motion, respawn prior, sight and sonar) and the levels.  Arguments as
        belief_update; with evidence, pmx_belief_weights_update_evidence."""
        first = int(first)
        count = self.n_envs - first if count is None else int(count)
        if count == 0:
            return belief, weights, levels
        self._check_belief(belief, count)
        self._check_weights(weights, count)
        self._check_levels(levels, count)
        red_dev = None
        if isinstance(team_red, torch.Tensor):
            assert team_red.shape == (self.n_envs,) and team_red.dtype == torch.uint8 and team_red.is_contiguous() and team_red.device == self.device
            red_dev, team_red = team_red.data_ptr(), 0
        if reset is not None:
            assert reset.shape == (self.n_envs,) and reset.dtype == torch.uint8 and reset.is_contiguous() and reset.device == self.device
        if sonar is not None:
            assert sonar.shape == (count, 2, 2) and sonar.dtype == torch.int8 and sonar.is_contiguous() and sonar.device == self.device
        with torch.cuda.device(self.device):
            if evidence is not None:
                self._check_evidence(evidence, count)
                _lib.call("pmx_belief_weights_update_evidence", self.handle, int(bool(team_red)), red_dev, first, count, int(sight_range),
                          int(rules), reset.data_ptr() if reset is not None else None, belief.data_ptr(),
                          sonar.data_ptr() if sonar is not None else None, weights.data_ptr(), levels.data_ptr(), evidence.data_ptr(),
                          _lib.stream(self.device))
                return belief, weights, levels
            _lib.call("pmx_belief_weights_update", self.handle, int(bool(team_red)), red_dev, first, count, int(sight_range),
                      reset.data_ptr() if reset is not None else None, belief.data_ptr(), sonar.data_ptr() if sonar is not None else None,
                      weights.data_ptr(), levels.data_ptr(), _lib.stream(self.device))
        return belief, weights, levels

    # -- belief evidence: side, eaten food, contact-only respawn (include/pmx.h, "Belief evidence") --------------------
    def new_belief_evidence(self, count=None):
        """The evidence rows for `count` envs (None: all) that ride beside a belief buffer: int32 [count, 36], zeroed (= not valid,
        what belief_evidence_init leaves).  Pass them as `evidence` to belief_update / belief_weights_update."""
        return torch.zeros((self.n_envs if count is None else int(count), _lib.EVIDENCE_WORDS), dtype=torch.int32, device=self.device)

    def _check_evidence(self, evidence, count):
        assert (evidence.shape == (count, _lib.EVIDENCE_WORDS) and evidence.dtype == torch.int32 and evidence.is_contiguous()
                and evidence.device == self.device)

    def belief_evidence_init(self, evidence, first=0, count=None):
        """pmx_belief_evidence_init on rows 0 .. count - 1 of `evidence` for the envs first .. first + count - 1: call it wherever
        belief_init / belief_weights_init is called on those rows."""
        first = int(first)
        count = self.n_envs - first if count is None else int(count)
        if count == 0:
            return evidence
        self._check_evidence(evidence, count)
        with torch.cuda.device(self.device):
            _lib.call("pmx_belief_evidence_init", self.handle, first, count, evidence.data_ptr(), _lib.stream(self.device))
        return evidence

    # -- episode statistics: an exact per-episode event record (include/pmx.h, "Episode statistics") -------------------
    def new_episode_stats(self, count=None):
        """The statistics buffer for `count` envs (None: all): int32 [48, count], WORD-major (word w of env first + r is
        stats[w, r]), zeroed.  Call episode_stats_init before the first step.  Needs an env created with auto_reset=False."""
        return torch.zeros((_lib.STATS_WORDS, self.n_envs if count is None else int(count)), dtype=torch.int32, device=self.device)

    def _check_stats(self, stats, count):
        assert (stats.shape == (_lib.STATS_WORDS, count) and stats.dtype == torch.int32 and stats.is_contiguous()
                and stats.device == self.device)

    def _stats_call(self, name, stats, first, count, *mid):
        first = int(first)
        count = self.n_envs - first if count is None else int(count)
        self._check_stats(stats, count)
        if count == 0:                                   # (an empty tensor has no address to pass)
            return stats
        with torch.cuda.device(self.device):
            _lib.call(name, self.handle, first, count, *mid, stats.data_ptr(), _lib.stream(self.device))
        return stats

    def episode_stats_init(self, stats, first=0, count=None):
        """pmx_episode_stats_init, after reset() or set_state() and before the first step(): the counters, TICKS and DONE of the
        rows 0 .. count - 1 (envs first .. first + count - 1) to zero, SCORE and the state words from the current state."""
        return self._stats_call("pmx_episode_stats_init", stats, first, count)

    def episode_stats_update(self, stats, done=None, first=0, count=None):
        """pmx_episode_stats_update, once after each step(): counts the tick's four sub-step transitions into every row that is
        not DONE.  done: uint8 [N] (step()'s done), non-zero = the row is DONE from now on and keeps every word."""
        if done is not None:
            assert done.shape == (self.n_envs,) and done.dtype == torch.uint8 and done.is_contiguous() and done.device == self.device
        return self._stats_call("pmx_episode_stats_update", stats, first, count, done.data_ptr() if done is not None else None)

    @staticmethod
    def episode_stats_dict(stats):
        """Named views of a statistics buffer: every counter of _lib.STAT_NAMES as [count, 4] (agent along the last axis), and
        ticks / score / done as [count]."""
        count = stats.shape[1]
        per = stats[:32].view(4, 8, count)
        out = {name: per[:, c].t() for c, name in enumerate(_lib.STAT_NAMES)}
        out.update(ticks=stats[_lib.STATS_W_TICKS], score=stats[_lib.STATS_W_SCORE], done=stats[_lib.STATS_W_DONE])
        return out

    # -- game records: a device log of every sub-step (include/pmx.h, "Game records") ------------------------------------
    def new_game_record(self, first=0, count=None, max_ticks=None):
        """The log buffers for the envs first .. first + count - 1 (count None: all from `first`) and up to max_ticks ticks (None:
        length + 1, a whole episode): a DeviceGameRecord.  Call game_record_init before the first step.  Needs an env created
        with auto_reset=False."""
        first = int(first)
        count = self.n_envs - first if count is None else int(count)
        max_ticks = self.length + 1 if max_ticks is None else int(max_ticks)
        fw = C.c_int32()
        _lib.call("pmx_game_record_words", self.handle, C.byref(fw))
        return DeviceGameRecord(self, first, count, max_ticks, fw.value)

    def _check_record(self, rec):
        for t, shape in ((rec.head, (_lib.RECORD_HEAD_WORDS, rec.count)), (rec.frames, (1 + 4 * rec.max_ticks, rec.frame_words, rec.count))):
            assert t.shape == shape and t.dtype == torch.int32 and t.is_contiguous() and t.device == self.device

    def game_record_init(self, rec):
        """pmx_game_record_init, after reset() or set_state() and before the first step(): LEN, DONE and OVERFLOW of every row
        to zero, LAYOUT from the env's layout, frame 0 from the current state."""
        self._check_record(rec)
        if rec.count == 0:                               # (an empty tensor has no address to pass)
            return rec
        with torch.cuda.device(self.device):
            _lib.call("pmx_game_record_init", self.handle, rec.first, rec.count, rec.max_ticks, rec.head.data_ptr(), rec.frames.data_ptr(),
                      _lib.stream(self.device))
        return rec

    def game_record_update(self, rec, done=None):
        """pmx_game_record_update, once after each step(): the tick's four sub-step states and their EVENT words into every row
        that is neither DONE nor full.  done: uint8 [N] (step()'s done), non-zero = the row is DONE from now on."""
        self._check_record(rec)
        if done is not None:
            assert done.shape == (self.n_envs,) and done.dtype == torch.uint8 and done.is_contiguous() and done.device == self.device
        if rec.count == 0:
            return rec
        with torch.cuda.device(self.device):
            _lib.call("pmx_game_record_update", self.handle, rec.first, rec.count, rec.max_ticks, done.data_ptr() if done is not None else None,
                      rec.head.data_ptr(), rec.frames.data_ptr(), _lib.stream(self.device))
        return rec

    # -- measurement ---------------------------------------------------------------------------------------------
    def profile_begin(self, max_launches):
        _lib.call("pmx_profile_begin", self.handle, int(max_launches))

    def set_tuning(self, key, value):
        """Launch tuning (pmx_set_tuning): "expand_alt" (0 = always the same sweep direction, -1 = the default alternation)
        and "fused_min_envs" (step() runs the tick in one launch from this many envs on, -1 = one workgroup per CU)."""
        _lib.call("pmx_set_tuning", self.handle, key.encode(), int(value))

    def last_step_fused(self):
        """True when the last step() ran the whole tick in one launch (pmx_last_step_fused)."""
        return bool(self.lib.pmx_last_step_fused(self.handle))

    def profile_end(self):
        """-> dict(rule_ms, rule_launches, expand_ms, expand_launches): summed kernel times from HIP events."""
        rm, em, rn, en = C.c_double(), C.c_double(), C.c_int32(), C.c_int32()
        _lib.call("pmx_profile_end", self.handle, C.byref(rm), C.byref(rn), C.byref(em), C.byref(en))
        return dict(rule_ms=rm.value, rule_launches=rn.value, expand_ms=em.value, expand_launches=en.value)

    # -- state exchange ------------------------------------------------------------------------------------------
    def get_state(self, first=0, count=None):
        count = self.n_envs - first if count is None else count
        arr = (_lib.State * count)()
        with torch.cuda.device(self.device):
            _lib.call("pmx_get_state", self.handle, first, count, arr, _lib.stream(self.device))
        return arr

    def set_state(self, states, first=0):
        count = len(states)
        arr = states if isinstance(states, C.Array) else (_lib.State * count)(*states)
        with torch.cuda.device(self.device):
            _lib.call("pmx_set_state", self.handle, first, count, arr, _lib.stream(self.device))

    def layout_indices(self):
        """The layout of the pool each env is on right now (int32 numpy array [n_envs])."""
        out = np.zeros(self.n_envs, np.int32)
        with torch.cuda.device(self.device):
            _lib.call("pmx_get_layout_index", self.handle, out.ctypes.data_as(C.POINTER(C.c_int32)), _lib.stream(self.device))
        return out

    def maze_distances(self, layout=0):
        """distanceCalculator.computeDistances for a layout -> (cells [n,2] int8, dist [n,n] uint8) on the GPU."""
        n = C.c_int32()
        with torch.cuda.device(self.device):
            _lib.call("pmx_maze_distances_layout", self.handle, layout, None, None, C.byref(n), _lib.stream(self.device))
            cells = torch.empty((n.value, 2), dtype=torch.int8, device=self.device)
            dist = torch.empty((n.value, n.value), dtype=torch.uint8, device=self.device)
            _lib.call("pmx_maze_distances_layout", self.handle, layout, cells.data_ptr(), dist.data_ptr(), C.byref(n), _lib.stream(self.device))
        return cells, dist


def make_state(pos, dir, pac, scared, carry, ret, food, caps, score, steps, H):
    s = _lib.State()
    for i in range(4):
        s.pos[i][0], s.pos[i][1] = int(pos[i][0]), int(pos[i][1])
        s.dir[i], s.pac[i], s.scared[i] = int(dir[i]), int(pac[i]), int(scared[i])
        s.carry[i], s.ret[i] = int(carry[i]), int(ret[i])
    for y in range(H):
        s.food[y], s.caps[y] = int(food[y]), int(caps[y])
    s.score, s.steps = int(score), int(steps)
    return s
