"""Vectorised MAPPO training loop on the GPU env (the rollout / GAE / PPO-update part of pacman_mappo_resnet.train()).

Per update (pacman_mappo_resnet.py:385-600), with N envs in lock-step instead of one:
  rollout  T ticks: canonicalise (red learners) and merge the two learner observations, sample both learners'
           actions from the actor and one value from the critic, step the env, add the heuristic shaping
           (:241-264, :513-522), store everything in DEVICE-resident buffers (:449-455 kept them on the CPU)
  GAE      pmx_gae over the [T][2N] series (:548-553)
  update   UPDATE_EPOCHS x minibatches of the flattened [T*N*2] samples through PPOLearner (:556-595)
Opponents: the in-kernel randomTeam, baselineTeam and approxQTeam bots (PMX_ACTION_RANDOM_LEGAL / PMX_ACTION_BASELINE_* /
PMX_ACTION_APPROXQ_*), the current network, or a frozen EMA snapshot from the opponent pool (:396-438; the A* / MCTS /
heuristic teams of the reference's curriculum are wall-clock-bounded searches and out of scope).
"""
import copy
from collections import deque
from fractions import Fraction

import numpy as np
import torch

from . import _lib, mappo
from .vec_env import PmxVecEnv

UPDATE_EPOCHS = 3                 # pacman_mappo_resnet.py:24
OPPONENT_POOL_SIZE = 80           # :32
OPPONENT_UPDATE_FREQ = 15         # :33


def shaping_from_agent_words(prev, cur):
    """compute_heuristic_shaping (pacman_mappo_resnet.py:251-264) from the compact self plane.
    prev/cur: int32 [...]: x | y << 8 | carry << 16 of the same agent in two consecutive observations.  float64."""
    px, py, pc = prev & 0xFF, (prev >> 8) & 0xFF, (prev >> 16) & 0xFFFF
    cx, cy = cur & 0xFF, (cur >> 8) & 0xFF
    moved = (px - cx).abs() + (py - cy).abs()
    living = -0.15
    died = (living - 0.4) - (0.15 * pc.to(torch.float64))
    out = torch.full(prev.shape, living, dtype=torch.float64, device=prev.device)
    out = torch.where(moved == 0, torch.full_like(out, living - 0.05), out)     # dist_moved < 0.1
    out = torch.where(moved > 1, died, out)                                     # dist_moved > 1.5
    return out


BOT_TEAMS = {"baseline": (_lib.ACTION_BASELINE_OFFENSE, _lib.ACTION_BASELINE_DEFENSE),      # createTeam: first index offensive,
             "approxq": (_lib.ACTION_APPROXQ_OFFENSE, _lib.ACTION_APPROXQ_DEFENSE)}         # second defensive
_OBS_CODES = {torch.float32: _lib.OBS_F32, torch.bfloat16: _lib.OBS_BF16, torch.uint8: _lib.OBS_U8}


def mix_plan(update_idx, curriculum_scale, n_envs, hard_bots, opponent_mode):
    """The opponents of ONE rollout spread over its envs (mix_opponents): [(mode, red, first, count), ...], contiguous env ranges
    from 0 in the order self, pool, each team of hard_bots, random.  The shares are the probabilities _pick_opponent draws
    with -- all random up to update 200 * scale; 5/6 hard teams (split evenly) and 1/6 random up to 800 * scale; then 0.40 self,
    0.20 pool and 0.40 x (5/6 hard, 1/6 random) -- or the single mode of a fixed opponent_mode.  Counts are rounded by largest
    remainder (ties to the earlier group) and sum to n_envs; empty groups are left out.  Bot and random groups play the learner
    blue, as the reference does; self and pool groups are split into a red first half (count // 2) and a blue rest, where the
    reference flips a coin.  A pure host function of its arguments: no draw, so every rank computes the same plan."""
    hard = [(b, Fraction(5, 6) / len(hard_bots)) for b in hard_bots] + [("random", Fraction(1, 6))]
    if opponent_mode != "curriculum":
        shares = [(opponent_mode, Fraction(1))]
    elif update_idx <= 200 * curriculum_scale:
        shares = [("random", Fraction(1))]
    elif update_idx <= 800 * curriculum_scale:
        shares = hard
    else:
        shares = [("self", Fraction(2, 5)), ("pool", Fraction(1, 5))] + [(m, Fraction(2, 5) * f) for m, f in hard]
    exact = [f * n_envs for _, f in shares]
    counts = [int(x) for x in exact]                            # floor (the shares are not negative)
    by_remainder = sorted(range(len(shares)), key=lambda i: (-(exact[i] - counts[i]), i))
    for i in by_remainder[:n_envs - sum(counts)]:
        counts[i] += 1
    plan, first = [], 0
    for (mode, _), c in zip(shares, counts):
        parts = [(True, c // 2), (False, c - c // 2)] if mode in ("self", "pool") else [(False, c)]
        for red, k in parts:
            if k:
                plan.append((mode, red, first, k))
                first += k
    return plan


def _plane_kernel_ok(*ts):
    return all(t.is_cuda and t.dim() == 4 and t.shape[1] == 8 and t.dtype in _OBS_CODES and t.dtype == ts[0].dtype for t in ts)


def merge_obs(a, b):
    """merge_obs_for_critic (pacman_mappo_resnet.py:267-274) on batches [N,8,H,W]: pmx_merge_obs on device tensors of an
    observation dtype, the torch formulation otherwise."""
    if _plane_kernel_ok(a, b) and a.shape == b.shape:
        a, b = a.contiguous(), b.contiguous()
        out = torch.empty_like(a)
        _lib.call("pmx_merge_obs", a.data_ptr(), b.data_ptr(), out.data_ptr(), a.shape[0], a.shape[2], a.shape[3], _OBS_CODES[a.dtype],
                  _lib.stream(a.device))
        return out
    m = a.clone()
    m[:, 1] = torch.maximum(torch.maximum(a[:, 1], b[:, 1]), torch.zeros_like(a[:, 1]))
    m[:, 4] = 0
    return m


def canonicalize_obs(o):
    """canonicalize_obs for a red learner (pacman_mappo_resnet.py:215-229): flip x, swap planes 2<->3, 6<->7; pmx_canonicalize_obs
    on device tensors [N,8,H,W] of an observation dtype, the torch formulation otherwise."""
    if _plane_kernel_ok(o):
        o = o.contiguous()
        out = torch.empty_like(o)
        _lib.call("pmx_canonicalize_obs", o.data_ptr(), out.data_ptr(), o.shape[0], o.shape[2], o.shape[3], _OBS_CODES[o.dtype],
                  _lib.stream(o.device))
        return out
    return torch.flip(o, dims=[-1])[..., [0, 1, 3, 2, 4, 5, 7, 6], :, :]


SIGHT_RANGE = 5                   # capture.py:69


def fog_obs(obs, sight_range=SIGHT_RANGE):
    """The contest's sight rule (GameState.makeObservation, capture.py:268-292) stated on observation planes [..., 8, H, W] of any
    element type, raw or canonical (planes 1, 4 and 5 keep their index under canonicalize_obs and the x-flip keeps Manhattan
    distances): the team's cells are the non-zero cells of planes 1 (self) and 4 (ally); an enemy cell of plane 5 is kept iff its
    Manhattan distance to one of them is <= sight_range.  Returns a new tensor; every other plane is unchanged.  The rollout
    gets the same planes from pmx_emit_team_obs_fog without a pass of its own; this is the path where no emission kernel runs
    (evaluate_vs_bots) and the statement that kernel is tested against."""
    H, W = obs.shape[-2], obs.shape[-1]
    ys = torch.arange(H, device=obs.device).repeat_interleave(W)
    xs = torch.arange(W, device=obs.device).repeat(H)
    within = ((ys[:, None] - ys[None, :]).abs() + (xs[:, None] - xs[None, :]).abs() <= int(sight_range)).to(torch.float32)   # [HW, HW]
    team = ((obs[..., 1, :, :] != 0) | (obs[..., 4, :, :] != 0)).reshape(obs.shape[:-3] + (H * W,)).to(torch.float32)
    seen = (team @ within > 0).reshape(obs.shape[:-3] + (H, W))      # cells within sight of a team cell (a count of at most H * W: exact)
    out = obs.clone()
    out[..., 5, :, :] = torch.where(seen, obs[..., 5, :, :], torch.zeros_like(obs[..., 5, :, :]))
    return out


class VecMAPPOTrainer:
    def __init__(self, layout, n_envs, horizon=32, minibatch=512, epochs=UPDATE_EPOCHS, obs_dtype=None,
                 device="cuda:0", seed=0, rank=0, world_size=1, process_group=None, total_updates=2000, length=300,
                 use_autocast=True, opponent="random", use_graph=False, algorithm="mappo", paired_minibatches=True, curriculum_scale=1.0,
                 env=None, redraw_layouts=False, force_collectives=False, hard_bots=("baseline",), mask_illegal=False,
                 mix_opponents=False, fog_of_war=False, sight_range=SIGHT_RANGE, belief=False, belief_weights=False, belief_evidence=False, fog_bots=False):
        self.device = torch.device(device)
        # fog_of_war: every policy input of the rollout (the learners', the self / pool opponent networks', the bootstrap
        # observation) comes from the fog entry points -- an enemy shows only within sight_range of one of the team's agents, the
        # contest's rule (capture.py:268-292) -- while merged_buf, the centralised critic's input, stays full-information.  Off: no
        # keyword is passed and the calls are the ones made before the flag existed
        self.fog_of_war = bool(fog_of_war)
        self.sight_range = int(sight_range)
        if self.fog_of_war and not 0 <= self.sight_range <= 64:
            raise ValueError(f"sight_range must be 0 .. 64, got {sight_range!r}")
        self._fog = {"sight_range": self.sight_range} if self.fog_of_war else {}
        # belief (needs fog_of_war): the env tracks, per learner slot and hidden enemy, the set of cells the enemy can be on
        # (pmx_belief_update: motion, respawn, the sight rule and the noisy sonar distances of the contest, capture.py:210-224) and
        # every policy input shows the sets in plane 5 (pmx_emit_team_obs_belief; a seen enemy is a one-cell set, so the sight
        # rule needs no pass of its own there).  One buffer for the learners; a second one, updated with the colours inverted,
        # when the opponent can be a network, which then sees what a learner of its colour sees.  The buffers are not part of
        # a checkpoint.  Off: no keyword is passed and no tracker call is made
        self.belief = bool(belief)
        if self.belief and not self.fog_of_war:
            raise ValueError("belief=True needs fog_of_war=True: without the sight rule no enemy is hidden and there is nothing to track")
        # belief_weights (needs fog_of_war and belief): beside every set the env keeps a weight per cell, the exact Bayes filter of
        # include/pmx.h "Belief weights", and plane 5 shows its levels 0 .. 16 in place of the sets' 0 / 1.  Every tracker call and
        # every belief emission of the rollout is then the weighted form (pmx_belief_weights_update / _init, pmx_emit_team_obs_weighted);
        # the two extra tensors ride along with each belief buffer and are not saved either.  Off: none of the new calls is made
        self.belief_weights = bool(belief_weights)
        if self.belief_weights and not (self.fog_of_war and self.belief):
            raise ValueError("belief_weights=True needs fog_of_war=True and belief=True: the weights refine the sets of the hidden enemies")
        # belief_evidence (needs fog_of_war and belief; with or without belief_weights): every update also uses what the observation
        # leaves public on a hidden enemy -- its side, a pellet it ate, and that it can only have died next to one of the team's
        # agents (pmx_belief_update_evidence / pmx_belief_weights_update_evidence).  Each belief buffer gets an evidence tensor,
        # initialised wherever the buffer is.  Plane 5 means what it meant, so nothing is saved and no flag is recorded
        self.belief_evidence = bool(belief_evidence)
        if self.belief_evidence and not (self.fog_of_war and self.belief):
            raise ValueError("belief_evidence=True needs fog_of_war=True and belief=True: the evidence narrows the sets of the hidden enemies")
        # fog_bots (needs fog_of_war and sight_range >= 1): the in-kernel bots obey the sight rule too (pmx_set_bot_sight at the
        # trainer's sight_range): a bot counts an enemy only within that range of itself or its mate, as the reference's bots do on
        # the contest's observation.  Set once, below, on an env created with bots.  No network input changes, so nothing is recorded
        self.fog_bots = bool(fog_bots)
        if self.fog_bots and not (self.fog_of_war and self.sight_range >= 1):
            raise ValueError("fog_bots=True needs fog_of_war=True and sight_range >= 1: the bots' rule is the learners' sight rule, and "
                             "sight 0 would need the hidden-enemy skip inside the transition itself")
        self.rank, self.world_size = rank, world_size
        # hard_bots: the in-kernel teams the curriculum draws its "hard" opponent from (the reference's hard teams are
        # baselineTeam, AstarTeam and approxQTeam, pacman_mappo_resnet.py:40-47); the default keeps the draws of earlier versions
        self.hard_bots = tuple(hard_bots)
        if not self.hard_bots or any(b not in BOT_TEAMS for b in self.hard_bots):
            raise ValueError(f"hard_bots must name in-kernel teams out of {sorted(BOT_TEAMS)}, got {hard_bots!r}")
        if obs_dtype is None:
            # byte planes on the bf16 path: the values are small integers, the fused actor tower reads bytes directly and
            # the rollout buffers are half the size; float32 planes (the reference's dtype) on the float32 path
            obs_dtype = "uint8" if use_autocast else "float32"
        # `env`: an already built vectorised env (anything with PmxVecEnv's surface).  The host-side tests pass a stand-in to
        # drive update() / the opponent schedule without a GPU; the product always builds the HIP env here, which raises
        # without a GPU
        self.env = env if env is not None else PmxVecEnv(
            layout, n_envs, length=length, reward_forLegalAction=True, defenceReward=True, auto_reset=True, obs_dtype=obs_dtype,
            device=self.device, seed=seed * 1000003 + rank, bots=opponent in BOT_TEAMS or opponent == "curriculum", redraw_layouts=redraw_layouts)
        if self.fog_bots and (opponent in BOT_TEAMS or opponent == "curriculum"):
            self.env.set_bot_sight(self.sight_range)
        self.N, self.T = n_envs, horizon
        self.minibatch, self.epochs = minibatch, epochs
        # "mappo": centralised critic on merge_obs_for_critic of the two learners (the reference).  "ippo": the same network
        # with the critic fed each agent's OWN observation (BASELINE config 5 names the comparison; the reference has no
        # IPPO, so this variant has no parity target -- SURVEY section 0)
        assert algorithm in ("mappo", "ippo")
        self.algorithm = algorithm
        # the reference's curriculum switches phases at updates 200 and 800 of 2 048 ticks each; a vectorised update holds
        # n_envs * horizon ticks, so the thresholds can be compressed (curriculum_scale 0.1 -> updates 20 and 80)
        self.curriculum_scale = float(curriculum_scale)
        # paired_minibatches: a minibatch is drawn as (env-tick) PAIRS, both learners of a pair together, so that the
        # centralised critic runs once per pair instead of once per agent sample (its input is the same merged observation
        # for both).  Every epoch is still a random permutation that visits each sample once and the loss of a minibatch is
        # the reference's; only the composition of the minibatches differs from the reference's independent shuffle of
        # agent samples (pacman_mappo_resnet.py:566-569).  False restores that shuffle.
        self.paired = bool(paired_minibatches) and algorithm == "mappo" and minibatch % 2 == 0
        self.graph_gather = True     # replayed steps assemble their minibatch with pmx_gather_rows (False: torch indexing + copies)
        self.total_updates = total_updates
        H, W = self.env.layout.height, self.env.layout.width
        self.obs_shape = (8, H, W)
        torch.manual_seed(seed)                                   # identical initial weights on every rank
        self.model = mappo.MAPPOAgent(self.obs_shape, 5, 2).to(self.device)
        self.autocast_dtype = torch.bfloat16 if use_autocast else None
        # force_collectives: issue the gradient all-reduce on a one-rank group too (bench.py rehearses the collective path on a
        # one-GPU box with it)
        self.learner = mappo.PPOLearner(self.model, process_group=process_group, world_size=world_size,
                                        autocast_dtype=self.autocast_dtype, force_collectives=force_collectives)
        if world_size > 1:
            import torch.distributed as dist
            dist.broadcast(self.learner.bucket.data, src=0, group=process_group)
            self.learner.ema.copy_(self.learner.bucket.data)
        self.opponent_model = mappo.MAPPOAgent(self.obs_shape, 5, 2).to(self.device)
        self.opponent_model.load_state_dict(self.model.state_dict())
        self.opponent_model.eval()
        self.opponent_pool = deque(maxlen=OPPONENT_POOL_SIZE)
        self.opponent_pool.append(self.learner.ema_state_dict())
        self.opponent_mode = opponent                              # "random" | "baseline" | "approxq" | "self" | "pool" | "curriculum"
        self.gen = torch.Generator(device=self.device).manual_seed(seed * 7919 + rank)   # action sampling, minibatch order: per rank
        # opponent mode / side / pool draws: the SAME stream on every rank, so that all ranks run the same kind of rollout
        # (an extra opponent forward per tick on some ranks only would make the others wait at every gradient all-reduce)
        self.np_rng = np.random.RandomState(seed * 31)
        dt, dev, N, T = self.env.obs_torch_dtype, self.device, n_envs, horizon
        self.obs_buf = torch.zeros((T, N, 2) + self.obs_shape, dtype=dt, device=dev)
        self.merged_buf = torch.zeros((T, N) + self.obs_shape, dtype=dt, device=dev)
        self.act_buf = torch.zeros((T, N, 2), dtype=torch.int64, device=dev)
        self.logp_buf = torch.zeros((T, N, 2), dtype=torch.float32, device=dev)
        self.rew_buf = torch.zeros((T, N, 2), dtype=torch.float32, device=dev)
        self.done_buf = torch.zeros((T, N, 2), dtype=torch.float32, device=dev)
        self.val_buf = torch.zeros((T, N, 2), dtype=torch.float32, device=dev)
        self.adv_buf = torch.zeros((T, N, 2), dtype=torch.float32, device=dev)
        self.ret_buf = torch.zeros((T, N, 2), dtype=torch.float32, device=dev)
        # mask_illegal: the policy samples over the legal actions only (the env's masks of the state it acts on, canonicalised, one
        # int32 word per learner and tick; mappo.sample_actions keyed by this seed and a counter that advances by one per call) and
        # the objective sees the same masks.  Off: the reference's path, no mask is read anywhere
        self.mask_illegal = bool(mask_illegal)
        if self.mask_illegal:
            self.legal_buf = torch.zeros((T, N, 2), dtype=torch.int32, device=dev)
            self.sample_seed = (seed + 0x9E3779B9 * rank) & 0xFFFFFFFF         # the trainer's seed; other ranks draw other streams
            self.sample_counter = 0
        # mix_opponents: every rollout realises the opponent mixture ACROSS its envs (mix_plan: contiguous groups of envs per
        # opponent, both colours where the reference flips a coin) instead of drawing one opponent and one colour for all of
        # them; the observations come from pmx_emit_team_obs_mixed.  Off: one pairing per rollout, the reference's scheme
        self.mix_opponents = bool(mix_opponents)
        starts = self.env.layout.starts.astype(np.int64)
        self.start_words = torch.tensor([int(starts[i, 0]) | (int(starts[i, 1]) << 8) for i in range(4)],
                                        dtype=torch.int32, device=dev)
        self.env.reset()
        if self.belief:
            self._belief = self._new_belief()
            self._belief_opp = self._new_belief() if opponent in ("self", "pool", "curriculum") else None
        self._acts = None                                          # persistent per-rollout tensors, allocated on first use
        self.prev_agent = self.start_words[None].expand(N, 4).clone()
        self.update_idx = 0
        self.stats = {}
        # Optional: replay the optimizer step from a hipGraph when every minibatch has the same shape (launch-bound at the
        # reference's 512 samples: 1.4x more optimizer steps/s).  Needs DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 (set by the package
        # on import; ROCm 7's graph packet capture corrupts a node after ~230 interleaved replays); the
        # update loop also checks the gradient norm once per update so that a non-finite policy is never sampled from.
        # (data parallel: the replayed step is one graph per gradient group with the eager RCCL all-reduce of that group between
        # them -- PPOLearner.capture -- so the collectives are the ones the eager step issues)
        if use_graph and not mappo.PPOLearner.graph_replay_safe():
            raise ValueError("use_graph needs DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 exported before HIP initialises (DESIGN.md section 5)")
        self.use_graph = bool(use_graph) and (horizon * n_envs * 2) % minibatch == 0
        self._graph_ready = False

    # ---------------------------------------------------------------------------------------------------------
    def _net_in(self, x):
        """Observation tensors are small integers: under autocast the network takes bytes or bf16 as they are (the fused
        actor tower reads either, the critic converts on entry), fp32 otherwise."""
        if self.autocast_dtype is not None:
            return x if x.dtype in (torch.uint8, torch.bfloat16) else x.to(torch.bfloat16)
        return x.float()

    def _freeze_tower_packs(self, on):
        """The rollout runs thousands of inference calls on frozen weights: pack the actor towers' parameters once, and the
        first head layer's weight with them (one pack per rollout, not one per tick)."""
        from . import actor_tower
        H, W = self.obs_shape[1], self.obs_shape[2]
        for m in (self.model, self.opponent_model):
            m.tower_pack = m.head_pack = None
            if on and self.autocast_dtype is not None and m.fused_tower and actor_tower.tower_supported(H, W):
                m.tower_pack = actor_tower.pack_params(actor_tower._tower_params(m.actor_backbone))
                lin = m.actor_head[0]
                if (m.fused_head and m.fused_head_max_batch > 0 and self.autocast_dtype == torch.bfloat16 and lin.weight.is_cuda and lin.weight.dtype == torch.float32
                        and lin.in_features == 32 * H * W and lin.out_features == 512):
                    m.head_pack = mappo.pack_actor_head(lin.weight, H, W)

    def _forward_policy(self, model, obs2, merged, want_value, legal=None):
        ctx = torch.autocast(device_type=self.device.type, dtype=self.autocast_dtype) if self.autocast_dtype else _NullCtx()
        with torch.no_grad(), ctx:
            if legal is None:
                a, lp = model.act(self._net_in(obs2.reshape((-1,) + self.obs_shape)), generator=self.gen)
            else:
                a, lp = model.act(self._net_in(obs2.reshape((-1,) + self.obs_shape)), legal=legal.reshape(-1), seed=self.sample_seed,
                                  counter=self.sample_counter)
                self.sample_counter += 1
            v = model.value(self._net_in(merged)).float() if want_value else None
        return a.view(-1, 2), lp.view(-1, 2), v

    # ---- belief buffers: [tensor, colour, evidence] with colour a host array [N]: 0 / 1 = the row tracks the enemies of a blue / red team,
    # -1 = start cells of the reset the constructor made, -2 = every open cell (both sound for either colour), 2 = the row missed
    # the last rollout's updates and is re-initialised before it is used again.  Under belief_weights the tensor is the triple
    # (sets, weights, levels), sliced and initialised together.  evidence: the env's evidence rows under belief_evidence, else None
    def _new_belief(self):
        b = self.env.new_belief()
        if self.belief_weights:
            b = (b,) + tuple(self.env.new_belief_weights())
        ev = self.env.new_belief_evidence() if self.belief_evidence else None
        self._belief_init(b, 0, evidence=ev)
        return [b, np.full(self.N, -1, np.int8), ev]

    def _belief_init(self, t, kind, lo=0, hi=None, evidence=None):
        """(re-)initialise the rows lo .. hi - 1 (None: all) of a buffer's tensor(s), and of its evidence, for the envs of the same
        indices"""
        if hi is None:
            kw = {}
        else:
            kw = {"first": lo, "count": hi - lo}
        if self.belief_weights:
            self.env.belief_weights_init(*(x if hi is None else x[lo:hi] for x in t), kind, **kw)
        else:
            self.env.belief_init(t if hi is None else t[lo:hi], kind, **kw)
        if evidence is not None:
            self.env.belief_evidence_init(evidence if hi is None else evidence[lo:hi], **kw)

    def _belief_kw(self, view):
        """the emission keyword that shows a buffer (rows 0 .. n - 1 as _belief_for returned them)"""
        return {"levels": view[2]} if self.belief_weights else {"belief": view}

    def _evidence_of(self, buf, n=None):
        """the evidence rows that go with the rows 0 .. n - 1 of a buffer (None without belief_evidence)"""
        return None if buf[2] is None else buf[2][:n]

    def _belief_update(self, red, view, done, evidence=None, **rows):
        if evidence is not None:
            rows["evidence"] = evidence
        if self.belief_weights:
            self.env.belief_weights_update(red, view[0], view[1], view[2], self.sight_range, reset=done, **rows)
        else:
            self.env.belief_update(red, view, self.sight_range, reset=done, **rows)

    def _belief_for(self, buf, want, n=None):
        """The buffer's tensor for a rollout whose rows 0 .. n - 1 (None: all) track the enemies of a team of colour want[row]:
        rows that tracked the other colour (or none, last rollout) are re-initialised to every open cell, run by run."""
        n = self.N if n is None else n
        t, colour, evidence = buf
        want = np.broadcast_to(np.asarray(want, np.int8), (self.N,))[:n]
        bad = np.nonzero((colour[:n] >= 0) & (colour[:n] != want))[0]
        if len(bad):
            cuts = np.nonzero(np.diff(bad) != 1)[0] + 1
            for run in np.split(bad, cuts):
                self._belief_init(t, 1, int(run[0]), int(run[-1]) + 1, evidence)
        colour[:n] = want
        colour[n:] = np.where(colour[n:] == -2, -2, 2)
        return tuple(x[:n] for x in t) if self.belief_weights else t[:n]

    def _hard_bot(self):
        """The hard in-kernel team of this rollout: one extra draw, made only when there is a choice."""
        if len(self.hard_bots) == 1:
            return self.hard_bots[0]
        return self.hard_bots[self.np_rng.randint(len(self.hard_bots))]

    def _pick_opponent(self):
        """The self-play part of the curriculum (pacman_mappo_resnet.py:396-438) with the opponents this build has."""
        mode = self.opponent_mode
        if mode == "curriculum":
            # :396-438 with the opponents this build has on the GPU: randomTeam first, then randomTeam / a hard team out of
            # hard_bots (the reference weights its "hard" teams, baselineTeam and approxQTeam among them, 5x), then 40 % self /
            # 20 % pool / 40 % bots
            if self.update_idx <= 200 * self.curriculum_scale:
                mode = "random"
            elif self.update_idx <= 800 * self.curriculum_scale:
                mode = self._hard_bot() if self.np_rng.rand() < 5.0 / 6.0 else "random"
            else:
                r = self.np_rng.rand()
                mode = "self" if r < 0.40 else ("pool" if r < 0.60 else (self._hard_bot() if self.np_rng.rand() < 5.0 / 6.0 else "random"))
        play_as_red = False
        if mode == "self":
            play_as_red = bool(self.np_rng.rand() > 0.5)
            self.opponent_model.load_state_dict(self.model.state_dict())
        elif mode == "pool":
            play_as_red = bool(self.np_rng.rand() > 0.5)
            self.opponent_model.load_state_dict(self.opponent_pool[self.np_rng.randint(len(self.opponent_pool))])
        return mode, play_as_red

    def rollout(self):
        """T ticks.  Per tick (pacman_mappo_resnet.py:461-546, N envs at once): the env itself writes the learners' (canonicalised)
        observations into obs_buf[t] and the merged critic input into merged_buf[t] (pmx_emit_team_obs -- no select / flip /
        copy / merge passes over the planes, and the four-agent observation tensor of pmx_step is not produced at all), the
        policy samples both learners' actions and one value, the env steps with the actions taken from a persistent tensor."""
        if self.mix_opponents:
            return self._rollout_mixed()
        env, N, T = self.env, self.N, self.T
        mode, red = self._pick_opponent()
        self._freeze_tower_packs(True)
        learner_ids = [0, 2] if red else [1, 3]
        opp_ids = [1, 3] if red else [0, 2]
        team = 0 if red else 1
        ep_ret = torch.zeros((), dtype=torch.float64, device=self.device)
        n_done = torch.zeros((), dtype=torch.int64, device=self.device)
        n_win = torch.zeros((), dtype=torch.int64, device=self.device)
        if self._acts is None:
            dt = self.obs_buf.dtype
            self._acts = torch.empty((N, 4), dtype=torch.int8, device=self.device)
            self._opp_obs = torch.empty((N, 2) + self.obs_shape, dtype=dt, device=self.device)
            self._boot_obs = torch.empty((N, 2) + self.obs_shape, dtype=dt, device=self.device)
            self._boot_merged = torch.empty((N,) + self.obs_shape, dtype=dt, device=self.device)
        acts = self._acts
        acts.fill_(_lib.ACTION_RANDOM_LEGAL)
        if mode in BOT_TEAMS:
            acts[:, opp_ids[0]], acts[:, opp_ids[1]] = BOT_TEAMS[mode]
        mappo_alg = self.algorithm == "mappo"
        masks = self.mask_illegal
        own, other = (slice(0, 4, 2), slice(1, 4, 2)) if red else (slice(1, 4, 2), slice(0, 4, 2))   # learner_ids / opp_ids of env.legal
        lg = None
        kw = okw = self._fog                                         # keywords of the learners' / the opponent network's emissions
        if self.belief:
            net = mode in ("self", "pool")
            bel, ev = self._belief_for(self._belief, int(red)), self._evidence_of(self._belief)
            kw = self._belief_kw(bel)
            if self._belief_opp is not None:
                obel, oev = self._belief_for(self._belief_opp, int(not red), None if net else 0), self._evidence_of(self._belief_opp, None if net else 0)
                okw = self._belief_kw(obel)
        for t in range(T):
            env.emit_team_obs(red, self.obs_buf[t], self.merged_buf[t] if mappo_alg else None, **kw)
            if masks:
                # env.legal: the masks of the state this tick acts on (written by the reset, the last step or its auto-reset)
                self.legal_buf[t].copy_(mappo.canonicalize_legal(env.legal[:, own], red))
                lg = self.legal_buf[t]
            if mappo_alg:
                a, lp, v = self._forward_policy(self.model, self.obs_buf[t], self.merged_buf[t], True, lg)
                self.val_buf[t].copy_(v[:, None].expand(N, 2))
            else:
                a, lp, v = self._forward_policy(self.model, self.obs_buf[t], self.obs_buf[t].view((-1,) + self.obs_shape), True, lg)
                self.val_buf[t].copy_(v.view(N, 2))
            self.act_buf[t].copy_(a)
            self.logp_buf[t].copy_(lp)
            acts[:, learner_ids] = mappo.canonicalize_action(a, red).to(torch.int8)
            if mode in ("self", "pool"):
                env.emit_team_obs(not red, self._opp_obs, None, **okw)            # the opponent is red when the learner is blue
                # (under masks the opponent, a copy of a policy trained under masks, samples the same way under its own ids' masks)
                oa, _, _ = self._forward_policy(self.opponent_model, self._opp_obs, None, False,
                                                mappo.canonicalize_legal(env.legal[:, other], not red) if masks else None)
                acts[:, opp_ids] = mappo.canonicalize_action(oa, not red).to(torch.int8)
            _, rew, done, info = env.step(acts, want_obs=False)
            if self.belief:
                self._belief_update(red, bel, done, ev)
                if net:
                    self._belief_update(not red, obel, done, oev)
            cur_agent = info["agent"]
            shp = shaping_from_agent_words(self.prev_agent[:, learner_ids], cur_agent[:, learner_ids])   # [N,2] f64
            team_reward = rew[:, team] + rew[:, team]                # sum over the two learners' (identical) rewards
            self.rew_buf[t].copy_((team_reward[:, None] + mappo.SHAPING_SCALE * shp).to(torch.float32))
            d = done.to(torch.bool)
            self.done_buf[t].copy_(done.to(torch.float32)[:, None].expand(N, 2))
            self.prev_agent = torch.where(d[:, None], self.start_words[None].expand(N, 4), cur_agent)
            ep_ret += team_reward.sum()
            n_done += d.sum()
            sc = info["score"]
            n_win += (d & ((sc > 0) if red else (sc < 0))).sum()
        # bootstrap value of the state after the last tick (:541-546)
        env.emit_team_obs(red, self._boot_obs, self._boot_merged if mappo_alg else None, **kw)
        ctx = torch.autocast(device_type=self.device.type, dtype=self.autocast_dtype) if self.autocast_dtype else _NullCtx()
        with torch.no_grad(), ctx:
            if mappo_alg:
                self.last_value = self.model.value(self._net_in(self._boot_merged)).float()[:, None].expand(N, 2).contiguous()
            else:
                self.last_value = self.model.value(self._net_in(self._boot_obs.view((-1,) + self.obs_shape))).float().view(N, 2)
        self._freeze_tower_packs(False)
        self.stats.update(opponent=mode, play_as_red=red, rollout_reward=ep_ret, episodes=n_done, wins=n_win)

    def _rollout_mixed(self):
        """rollout() with the pairing chosen per env (mix_opponents): the plan's groups play side by side in one rollout.  The
        learners' colour is a [N] tensor, so the frame helpers take their per-env forms and the reward, shaping and win test
        pick their columns by it; a stored sample is canonical and does not know its env's colour, so the buffers, the GAE and
        update() are those of the default path.  Network opponents (self: the current model, pool: ONE snapshot per rollout)
        fill the first envs and get their observations from a second emission over that range with the colours inverted."""
        env, N, T = self.env, self.N, self.T
        plan = mix_plan(self.update_idx, self.curriculum_scale, N, self.hard_bots, self.opponent_mode)
        n_self = sum(c for m, _, _, c in plan if m == "self")
        n_pool = sum(c for m, _, _, c in plan if m == "pool")
        n_net = n_self + n_pool                                    # self then pool: envs [0, n_self) and [n_self, n_net)
        if n_pool:                                                 # the rollout's only draw, the same on every rank
            self.opponent_model.load_state_dict(self.opponent_pool[self.np_rng.randint(len(self.opponent_pool))])
        self._freeze_tower_packs(True)
        dev = self.device
        if self._acts is None:
            dt = self.obs_buf.dtype
            self._acts = torch.empty((N, 4), dtype=torch.int8, device=dev)
            self._opp_obs = torch.empty((N, 2) + self.obs_shape, dtype=dt, device=dev)
            self._boot_obs = torch.empty((N, 2) + self.obs_shape, dtype=dt, device=dev)
            self._boot_merged = torch.empty((N,) + self.obs_shape, dtype=dt, device=dev)
        red_host = np.zeros(N, np.uint8)
        acts_host = np.full((N, 4), _lib.ACTION_RANDOM_LEGAL, np.int8)
        for mode, red, first, count in plan:
            red_host[first:first + count] = red
            if mode in BOT_TEAMS:                                  # (bot groups are blue: the bots play agents 0 and 2)
                acts_host[first:first + count, 1 if red else 0], acts_host[first:first + count, 3 if red else 2] = BOT_TEAMS[mode]
        red_u8 = torch.from_numpy(red_host).to(dev)
        inv_u8 = 1 - red_u8
        red_b = red_u8.to(torch.bool)
        acts = self._acts
        acts.copy_(torch.from_numpy(acts_host))
        self.mix_groups, self.team_red = plan, red_u8
        opp_obs = self._opp_obs[:n_net]
        ep_ret = torch.zeros((), dtype=torch.float64, device=dev)
        done_env = torch.zeros(N, dtype=torch.int64, device=dev)
        win_env = torch.zeros(N, dtype=torch.int64, device=dev)
        mappo_alg = self.algorithm == "mappo"
        masks = self.mask_illegal
        lg = None
        kw = okw = self._fog                                         # keywords of the learners' / the opponent networks' emissions
        if self.belief:
            bel, ev = self._belief_for(self._belief, red_host), self._evidence_of(self._belief)
            kw = self._belief_kw(bel)
            if self._belief_opp is not None:
                obel, oev = self._belief_for(self._belief_opp, 1 - red_host, n_net), self._evidence_of(self._belief_opp, n_net)
                okw = self._belief_kw(obel)
        for t in range(T):
            env.emit_team_obs_mixed(red_u8, self.obs_buf[t], self.merged_buf[t] if mappo_alg else None, **kw)
            if masks:
                self.legal_buf[t].copy_(mappo.canonicalize_legal(mappo.team_columns(env.legal, red_u8), red_u8))
                lg = self.legal_buf[t]
            if mappo_alg:
                a, lp, v = self._forward_policy(self.model, self.obs_buf[t], self.merged_buf[t], True, lg)
                self.val_buf[t].copy_(v[:, None].expand(N, 2))
            else:
                a, lp, v = self._forward_policy(self.model, self.obs_buf[t], self.obs_buf[t].view((-1,) + self.obs_shape), True, lg)
                self.val_buf[t].copy_(v.view(N, 2))
            self.act_buf[t].copy_(a)
            self.logp_buf[t].copy_(lp)
            mappo.set_team_columns(acts, red_u8, mappo.canonicalize_action(a, red_u8))
            if n_net:
                env.emit_team_obs_mixed(inv_u8, opp_obs, None, 0, n_net, **okw)           # the opponent is red where the learner is blue
                olg = mappo.canonicalize_legal(mappo.team_columns(env.legal, red_u8, opponents=True), inv_u8) if masks else None
                for model, lo, hi in ((self.model, 0, n_self), (self.opponent_model, n_self, n_net)):
                    if hi > lo:
                        oa, _, _ = self._forward_policy(model, opp_obs[lo:hi], None, False, olg[lo:hi] if masks else None)
                        mappo.set_team_columns(acts[lo:hi], red_u8[lo:hi], mappo.canonicalize_action(oa, inv_u8[lo:hi]), opponents=True)
            _, rew, done, info = env.step(acts, want_obs=False)
            if self.belief:
                self._belief_update(red_u8, bel, done, ev)
                if n_net:
                    self._belief_update(inv_u8, obel, done, oev, first=0, count=n_net)
            cur_agent = info["agent"]
            shp = shaping_from_agent_words(mappo.team_columns(self.prev_agent, red_u8), mappo.team_columns(cur_agent, red_u8))   # [N,2] f64
            own = torch.where(red_b, rew[:, 0], rew[:, 1])
            team_reward = own + own                                  # sum over the two learners' (identical) rewards
            self.rew_buf[t].copy_((team_reward[:, None] + mappo.SHAPING_SCALE * shp).to(torch.float32))
            d = done.to(torch.bool)
            self.done_buf[t].copy_(done.to(torch.float32)[:, None].expand(N, 2))
            self.prev_agent = torch.where(d[:, None], self.start_words[None].expand(N, 4), cur_agent)
            ep_ret += team_reward.sum()
            done_env += d
            sc = info["score"]
            win_env += d & torch.where(red_b, sc > 0, sc < 0)
        # bootstrap value of the state after the last tick (:541-546)
        env.emit_team_obs_mixed(red_u8, self._boot_obs, self._boot_merged if mappo_alg else None, **kw)
        ctx = torch.autocast(device_type=self.device.type, dtype=self.autocast_dtype) if self.autocast_dtype else _NullCtx()
        with torch.no_grad(), ctx:
            if mappo_alg:
                self.last_value = self.model.value(self._net_in(self._boot_merged)).float()[:, None].expand(N, 2).contiguous()
            else:
                self.last_value = self.model.value(self._net_in(self._boot_obs.view((-1,) + self.obs_shape))).float().view(N, 2)
        self._freeze_tower_packs(False)
        by_mode = {}
        for mode, _, first, count in plan:
            e, w = by_mode.get(mode, (0, 0))
            by_mode[mode] = (e + done_env[first:first + count].sum(), w + win_env[first:first + count].sum())
        self.stats.update(opponent="mixed", play_as_red=None, rollout_reward=ep_ret, episodes=done_env.sum(), wins=win_env.sum(),
                          episodes_by_mode={m: e for m, (e, _) in by_mode.items()}, wins_by_mode={m: w for m, (_, w) in by_mode.items()})

    def compute_gae(self):
        T, n = self.T, self.N * 2
        last = self.last_value.contiguous()                         # [N, 2]
        _lib.call("pmx_gae", self.rew_buf.data_ptr(), self.val_buf.data_ptr(), self.done_buf.data_ptr(), last.data_ptr(), T, n, mappo.GAMMA,
                  mappo.GAE_LAMBDA, self.adv_buf.data_ptr(), self.ret_buf.data_ptr(), _lib.stream(self.device))

    def update(self, max_steps=None):
        """The PPO epochs over the rollout buffers.  max_steps stops after that many optimizer steps (warm-up runs only)."""
        lr, ent_coef, clip_eps = mappo.schedule(self.update_idx, self.total_updates)
        self.learner.set_lr(lr)
        S = self.T * self.N * 2
        obs = self.obs_buf.view((S,) + self.obs_shape)
        merged = self.merged_buf.view((self.T * self.N,) + self.obs_shape)
        act, logp = self.act_buf.view(S), self.logp_buf.view(S)
        adv, ret = self.adv_buf.view(S), self.ret_buf.view(S)
        legal = self.legal_buf.view(S) if self.mask_illegal else None
        agg = None
        steps = 0
        snap = None
        # the one-launch minibatch gather needs the rollout tensors in the very type the graph's inputs have
        gather = bool(self.use_graph and self.graph_gather and self.paired and self.device.type == "cuda" and S % self.minibatch == 0
                      and self._net_in(obs[:1]).dtype == obs.dtype and self._net_in(merged[:1]).dtype == merged.dtype)
        if self.use_graph:      # a bad replay must not leave NaNs in the weights, the Adam moments and the EMA: keep a copy to go back to
            snap = self.learner.snapshot()
        for _ in range(self.epochs):
            if self.paired:
                pperm = torch.randperm(S // 2, device=self.device, generator=self.gen)
            else:
                perm = torch.randperm(S, device=self.device, generator=self.gen)
            for s0 in range(0, S, self.minibatch):
                if self.paired:
                    pr = pperm[s0 // 2:(s0 + self.minibatch) // 2]
                else:
                    mb = perm[s0:s0 + self.minibatch]
                if self.use_graph and not self._graph_ready:
                    self.learner.capture(self.minibatch, self.obs_shape, self._net_in(obs[:1]).dtype,
                                         clip_eps, ent_coef, merged_batch=self.minibatch // 2 if self.paired else None,
                                         **({"masked": True} if legal is not None else {}))
                    self._graph_ready = True
                if gather:
                    # replayed step, paired minibatch: one gather launch into the graph's inputs, reports summed inside the graph
                    if steps == 0:
                        self.learner.reset_report_sums()
                    src = {"obs": obs, "merged": merged, "act": act, "logp": logp, "adv": adv, "ret": ret}
                    rows = {"obs": 2, "merged": 1, "act": 2, "logp": 2, "adv": 2, "ret": 2}
                    if legal is not None:
                        src["legal"], rows["legal"] = legal, 2
                    self.learner.update_minibatch_graph_gather(src, pr, rows, clip_eps, ent_coef)
                    steps += 1
                    if max_steps is not None and steps >= max_steps:
                        break
                    continue
                mb = torch.stack((2 * pr, 2 * pr + 1), dim=1).reshape(-1) if self.paired else mb   # rows 2k, 2k+1 = the two learners of pair k
                step = self.learner.update_minibatch_graph if self.use_graph else self.learner.update_minibatch
                critic_in = merged[pr] if self.paired else (merged[mb // 2] if self.algorithm == "mappo" else obs[mb])
                st = step(self._net_in(obs[mb]), self._net_in(critic_in), act[mb], logp[mb], adv[mb], ret[mb], clip_eps, ent_coef,
                          **({"legal": legal[mb]} if legal is not None else {}))
                steps += 1
                agg = {k: v.clone() for k, v in st.items()} if agg is None else {k: agg[k] + st[k] for k in agg}
                if max_steps is not None and steps >= max_steps:
                    break
            if max_steps is not None and steps >= max_steps:
                break
        if gather:
            agg = self.learner.report_sums()
        self.stats.update({k: v / steps for k, v in agg.items()})
        if self.use_graph and not bool(torch.isfinite(self.stats["grad_norm"]).item()):
            self.learner.restore(snap)
            raise RuntimeError("non-finite gradient norm from the graph-replayed optimizer step; the learner was restored to "
                               "its state before this update")
        self.stats.update(lr=lr, ent_coef=ent_coef, clip_eps=clip_eps, optimizer_steps=steps)
        if self.update_idx % OPPONENT_UPDATE_FREQ == 0:
            self.opponent_pool.append(self.learner.ema_state_dict())
        self.update_idx += 1

    def train_update(self):
        self.rollout()
        self.compute_gae()
        self.update()
        return self.stats

    def save_ema(self, path):
        """The reference's checkpoint: EMA weights only (pacman_mappo_resnet.py:647-651)."""
        torch.save(self.learner.ema_state_dict(), path)

    def save_full(self, path):
        """Full resume state, which the reference lacks: weights, EMA, Adam moments, opponent pool,
        counters and both random streams -- tensors, numbers and strings only, so that it loads with weights_only=True.
        The games themselves are not saved: a resumed run starts its envs from fresh episodes."""
        kind, keys, pos, has_gauss, cached = self.np_rng.get_state()
        # (the mask flag and the sampler's counter are written only when the flag is on: a file of the default path is the one
        # earlier versions wrote)
        extra = {"mask_illegal": 1, "sample_counter": int(self.sample_counter)} if self.mask_illegal else {}
        if self.mix_opponents:                                           # (likewise written only when on)
            extra["mix_opponents"] = 1
        if self.fog_of_war:                                              # (likewise)
            extra["fog_of_war"], extra["sight_range"] = 1, int(self.sight_range)
        if self.belief_weights:                                          # (likewise: the policy was trained on levels, not on 0 / 1)
            extra["belief_weights"] = 1
        torch.save({**extra, "data": self.learner.bucket.data, "ema": self.learner.ema, "exp_avg": self.learner.exp_avg,
                    "exp_avg_sq": self.learner.exp_avg_sq, "step": int(self.learner.step_count), "update": int(self.update_idx),
                    "total_updates": int(self.total_updates), "pool": list(self.opponent_pool), "gen": self.gen.get_state(),
                    "hard_bots": list(self.hard_bots),
                    "np_rng": {"kind": str(kind), "keys": torch.from_numpy(np.asarray(keys, dtype=np.int64)), "pos": int(pos),
                               "has_gauss": int(has_gauss), "cached_gaussian": float(cached)}}, path)

    def load_full(self, path):
        ck = torch.load(path, map_location=self.device, weights_only=True)
        need = ("data", "ema", "exp_avg", "exp_avg_sq", "step", "update", "total_updates", "pool", "gen", "np_rng")
        if not isinstance(ck, dict) or any(k not in ck for k in need) or not isinstance(ck["np_rng"], dict) or "keys" not in ck["np_rng"]:
            raise ValueError(f"{path}: not a full-resume checkpoint of this version (save_full writes the keys {', '.join(need)}; "
                             "checkpoints written before `total_updates` and the tensor-valued `np_rng` were added are not supported)")
        if bool(ck.get("mask_illegal", 0)) != self.mask_illegal:          # (no key: written with the flag off)
            raise ValueError(f"checkpoint was written with mask_illegal={bool(ck.get('mask_illegal', 0))}, this trainer has "
                             f"mask_illegal={self.mask_illegal}: a policy trained under masks is sampled under masks")
        if bool(ck.get("mix_opponents", 0)) != self.mix_opponents:        # (no key: written with the flag off)
            raise ValueError(f"checkpoint was written with mix_opponents={bool(ck.get('mix_opponents', 0))}, this trainer has "
                             f"mix_opponents={self.mix_opponents}: the opponent draws of the two schemes do not continue one another")
        ck_fog = (bool(ck.get("fog_of_war", 0)), int(ck.get("sight_range", self.sight_range)))      # (no key: written with the flag off)
        if ck_fog[0] != self.fog_of_war or (self.fog_of_war and ck_fog[1] != self.sight_range):
            raise ValueError(f"checkpoint was written with fog_of_war={ck_fog[0]}" + (f", sight_range={ck_fog[1]}" if ck_fog[0] else "") +
                             f", this trainer has fog_of_war={self.fog_of_war}" + (f", sight_range={self.sight_range}" if self.fog_of_war else "") +
                             ": a policy trained on fogged planes is fed fogged planes")
        if bool(ck.get("belief_weights", 0)) != self.belief_weights:      # (no key: written with the flag off)
            raise ValueError(f"checkpoint was written with belief_weights={bool(ck.get('belief_weights', 0))}, this trainer has "
                             f"belief_weights={self.belief_weights}: a policy trained on the levels 0 .. 16 in plane 5 is fed levels")
        if int(ck["total_updates"]) != int(self.total_updates):
            raise ValueError(f"checkpoint was written for a schedule of {ck['total_updates']} updates, this trainer has {self.total_updates}")
        self.learner.restore(ck)                                         # (weights, Adam moments, EMA and step count: the same keys)
        self.update_idx = int(ck["update"])
        self.opponent_pool = deque(ck["pool"], maxlen=OPPONENT_POOL_SIZE)
        self.gen.set_state(ck["gen"].cpu())
        self.hard_bots = tuple(ck.get("hard_bots", ("baseline",)))       # files written before hard_bots existed: the default
        if self.mask_illegal:
            self.sample_counter = int(ck["sample_counter"])
        r = ck["np_rng"]
        self.np_rng.set_state((r["kind"], r["keys"].cpu().numpy().astype(np.uint32), int(r["pos"]), int(r["has_gauss"]),
                               float(r["cached_gaussian"])))
        if self.belief:                                                  # the sets are not saved: a resumed run knows the board only
            for buf in (self._belief, self._belief_opp):
                if buf is not None:
                    self._belief_init(buf[0], 1, evidence=buf[2])
                    buf[1][:] = -2


def evaluate_vs_bots(model, num_episodes=20, layout_file="bloxCapture", teams=("baselineTeam", "randomTeam"), length=300,
                     device="cuda:0", fog_of_war=False, sight_range=SIGHT_RANGE, belief=False, belief_weights=False, fog_bots=False):
    """evaluate_vs_bots (pacman_mappo_resnet.py:293-337): a fresh env per episode against host CaptureAgent bots (red),
    the learner plays blue with argmax actions; returns (mean return, std, win rate), a win being final score < 0.
    The reference cycles through its A*/approx-Q/baseline/MCTS teams; here through the team files this build ships.
    fog_of_war: the learner's planes go through fog_obs (the host bots keep the full state the env gives them unless fog_bots).
    fog_bots (needs fog_of_war and sight_range == 5, the contest's constant the host GameState.makeObservation uses): every host
    bot is asked on its own observation, gymPacMan_parallel_env(fog_bots=True)."""
    if fog_bots and not fog_of_war:
        raise ValueError("fog_bots=True needs fog_of_war=True")
    if fog_bots and int(sight_range) != SIGHT_RANGE:
        raise ValueError(f"fog_bots=True on the host-bot path uses the contest's SIGHT_RANGE = {SIGHT_RANGE}, got sight_range={sight_range!r}")
    if belief_weights:
        raise ValueError("evaluate_vs_bots has no belief tracker (no emission kernel runs on the host-bot path): evaluate a policy "
                         "trained with belief_weights=True with evaluate_vectorized(belief_weights=True)")
    if belief:
        raise ValueError("evaluate_vs_bots has no belief tracker (no emission kernel runs on the host-bot path): evaluate a policy "
                         "trained with belief=True with evaluate_vectorized(belief=True)")
    from .gym_env import gymPacMan_parallel_env
    was_training = model.training
    model.eval()
    returns, wins = [], 0
    learner_ids = [1, 3]
    for ep in range(num_episodes):
        env = gymPacMan_parallel_env(layout_file=layout_file, display=False, reward_forLegalAction=True, defenceReward=True,
                                     length=length, enemieName=teams[ep % len(teams)], self_play=False, device=device,
                                     **({"fog_bots": True} if fog_bots else {}))
        obs_dict, _ = env.reset()
        ep_ret, done = 0.0, False
        while not done:
            lo = torch.stack([obs_dict[env.agents[i]].float() for i in learner_ids])
            if fog_of_war:
                lo = fog_obs(lo, sight_range)
            with torch.no_grad():
                acts = model.get_deterministic_action(lo.to(next(model.parameters()).device)).cpu()
            obs_dict, rewards, dones, _ = env.step({env.agents[a]: int(acts[k]) for k, a in enumerate(learner_ids)})
            ep_ret += sum(rewards[env.agents[i]] for i in learner_ids)
            done = any(dones.values())
        returns.append(ep_ret)
        wins += int(env.game.state.data.score < 0)
        env.close()
    if was_training:
        model.train()
    return float(np.mean(returns)), float(np.std(returns)), wins / num_episodes


@torch.no_grad()
def evaluate_vectorized(model, layout="bloxCapture", n_envs=1024, opponent="baseline", length=300, device="cuda:0", seed=0,
                        autocast=True, mask_illegal=False, side="blue", fog_of_war=False, sight_range=SIGHT_RANGE, belief=False, belief_weights=False,
                        belief_evidence=False, fog_bots=False):
    """evaluate_vs_bots (pacman_mappo_resnet.py:293-337) for n_envs episodes at once: the learner plays blue with argmax
    actions against the in-kernel randomTeam / baselineTeam / approxQTeam (opponent "random" / "baseline" / "approxq"), one episode per env (an env stops counting at its first done).
    Returns (mean episode return of the learner team as the reference sums it, std, win rate = share with final score < 0).
    mask_illegal: the argmax runs over the legal actions only (a policy trained with the trainer's mask_illegal).
    side: "blue" as above; "red": the learner plays red and the bots blue; "both": red in the first half of the envs, blue in
    the rest (a policy trained with mix_opponents plays both colours).  A red learner's win is a final score > 0.
    fog_of_war: the policy sees an enemy only within sight_range of one of its two agents (pmx_emit_team_obs_mixed_fog); every
    side, blue included, then runs the emission-based loop.  The in-kernel bots keep the full state unless fog_bots.
    fog_bots (needs fog_of_war and sight_range >= 1): the in-kernel bots obey the same sight rule (pmx_set_bot_sight at sight_range).
    belief (needs fog_of_war): plane 5 shows the tracker's sets (pmx_belief_update after every step, pmx_emit_team_obs_mixed_belief),
    the inputs of a policy trained with the trainer's belief=True.
    belief_weights (needs fog_of_war and belief): plane 5 shows the weighted tracker's levels (pmx_belief_weights_update,
    pmx_emit_team_obs_mixed_weighted), the inputs of a policy trained with the trainer's belief_weights=True.
    belief_evidence (needs fog_of_war and belief): the updates are the evidence forms, as under the trainer's belief_evidence=True."""
    if side not in ("blue", "red", "both"):
        raise ValueError(f"side must be blue, red or both, got {side!r}")
    if belief and not fog_of_war:
        raise ValueError("belief=True needs fog_of_war=True")
    if belief_weights and not (fog_of_war and belief):
        raise ValueError("belief_weights=True needs fog_of_war=True and belief=True")
    if belief_evidence and not (fog_of_war and belief):
        raise ValueError("belief_evidence=True needs fog_of_war=True and belief=True")
    if fog_bots and not (fog_of_war and int(sight_range) >= 1):
        raise ValueError("fog_bots=True needs fog_of_war=True and sight_range >= 1")
    if side != "blue" or fog_of_war:
        return _evaluate_sides(model, layout, n_envs, opponent, length, device, seed, autocast, mask_illegal, side,
                               int(sight_range) if fog_of_war else None, **({"belief": True} if belief else {}), **({"belief_weights": True} if belief_weights else {}),
                               **({"belief_evidence": True} if belief_evidence else {}), **({"fog_bots": True} if fog_bots else {}))
    dev = torch.device(device)
    env = PmxVecEnv(layout, n_envs, length=length, auto_reset=True, obs_dtype="bfloat16" if autocast else "float32", device=dev,
                    seed=seed, bots=opponent in BOT_TEAMS)
    obs, legal = env.reset()
    was_training = model.training
    model.eval()
    alive = torch.ones(n_envs, dtype=torch.bool, device=dev)
    ret = torch.zeros(n_envs, dtype=torch.float64, device=dev)
    final = torch.zeros(n_envs, dtype=torch.int32, device=dev)
    opp = BOT_TEAMS.get(opponent, (_lib.ACTION_RANDOM_LEGAL,) * 2)
    ctx = torch.autocast(device_type=dev.type, dtype=torch.bfloat16) if autocast else _NullCtx()
    for _ in range(length + 1):
        lo = obs[:, [1, 3]].reshape((-1,) + tuple(obs.shape[2:]))
        with ctx:
            if mask_illegal:
                a = model.get_deterministic_action(lo.to(torch.bfloat16) if autocast else lo.float(),
                                                   legal=mappo.canonicalize_legal(legal[:, 1::2], False).reshape(-1)).view(n_envs, 2)
            else:
                a = model.get_deterministic_action(lo.to(torch.bfloat16) if autocast else lo.float()).view(n_envs, 2)
        acts = torch.empty((n_envs, 4), dtype=torch.int8, device=dev)
        acts[:, 0], acts[:, 2] = opp[0], opp[1]
        acts[:, [1, 3]] = a.to(torch.int8)
        obs, rew, done, info = env.step(acts)
        legal = info["legal_actions"]
        ret += torch.where(alive, rew[:, 1] + rew[:, 1], torch.zeros_like(ret))     # sum over both learners' rewards (:328)
        d = done.to(torch.bool) & alive
        final = torch.where(d, info["score"], final)
        alive &= ~d
        if not bool(alive.any()):
            break
    env.close()
    if was_training:
        model.train()
    return float(ret.mean()), float(ret.std()), float((final < 0).double().mean())


def _evaluate_sides(model, layout, n_envs, opponent, length, device, seed, autocast, mask_illegal, side, sight_range=None, belief=False,
                    belief_weights=False, belief_evidence=False, fog_bots=False):
    """evaluate_vectorized with the learner's colour chosen per env: observations from pmx_emit_team_obs_mixed (canonical, so the
    policy sees a red game as it was trained to), actions and masks through the per-env frame helpers.  sight_range (an int): the
    fog form of the emission; with belief the belief form, the sets advanced after every step; with belief_weights the weighted
    forms of both; with belief_evidence the updates are the evidence forms; with fog_bots (needs sight_range >= 1) the in-kernel
    bots obey the sight rule at sight_range."""
    if fog_bots and (sight_range is None or int(sight_range) < 1):
        raise ValueError("fog_bots=True needs fog_of_war=True and sight_range >= 1")
    dev = torch.device(device)
    env = PmxVecEnv(layout, n_envs, length=length, auto_reset=True, obs_dtype="bfloat16" if autocast else "float32", device=dev,
                    seed=seed, bots=opponent in BOT_TEAMS)
    if fog_bots and opponent in BOT_TEAMS:
        env.set_bot_sight(int(sight_range))
    env.reset(want_obs=False)
    was_training = model.training
    model.eval()
    red = torch.zeros(n_envs, dtype=torch.uint8, device=dev)
    red[:{"red": n_envs, "both": n_envs // 2, "blue": 0}[side]] = 1
    red_b = red.to(torch.bool)
    alive = torch.ones(n_envs, dtype=torch.bool, device=dev)
    ret = torch.zeros(n_envs, dtype=torch.float64, device=dev)
    final = torch.zeros(n_envs, dtype=torch.int32, device=dev)
    opp = BOT_TEAMS.get(opponent, (_lib.ACTION_RANDOM_LEGAL,) * 2)
    acts = torch.empty((n_envs, 4), dtype=torch.int8, device=dev)
    mappo.set_team_columns(acts, red, torch.tensor(opp, dtype=torch.int8, device=dev)[None].expand(n_envs, 2), opponents=True)
    team_obs = torch.empty((n_envs, 2) + env.obs_shape, dtype=env.obs_torch_dtype, device=dev)
    ctx = torch.autocast(device_type=dev.type, dtype=torch.bfloat16) if autocast else _NullCtx()
    kw = {} if sight_range is None else {"sight_range": sight_range}
    if belief_weights:
        bel, wts, lev = env.belief_weights_init(env.new_belief(), *env.new_belief_weights(), 0)
        kw = {"levels": lev}
    elif belief:
        bel = env.belief_init(env.new_belief(), 0)
        kw = {"belief": bel}
    ekw = {"evidence": env.belief_evidence_init(env.new_belief_evidence())} if belief_evidence else {}
    for _ in range(length + 1):
        env.emit_team_obs_mixed(red, team_obs, **kw)
        lo = team_obs.view((-1,) + env.obs_shape)
        with ctx:
            if mask_illegal:
                lg = mappo.canonicalize_legal(mappo.team_columns(env.legal, red), red).reshape(-1)
                a = model.get_deterministic_action(lo, legal=lg).view(n_envs, 2)
            else:
                a = model.get_deterministic_action(lo).view(n_envs, 2)
        mappo.set_team_columns(acts, red, mappo.canonicalize_action(a, red))
        _, rew, done, info = env.step(acts, want_obs=False)
        if belief_weights:
            env.belief_weights_update(red, bel, wts, lev, sight_range, reset=done, **ekw)
        elif belief:
            env.belief_update(red, bel, sight_range, reset=done, **ekw)
        own = torch.where(red_b, rew[:, 0], rew[:, 1])
        ret += torch.where(alive, own + own, torch.zeros_like(ret))                 # sum over both learners' rewards (:328)
        d = done.to(torch.bool) & alive
        final = torch.where(d, info["score"], final)
        alive &= ~d
        if not bool(alive.any()):
            break
    env.close()
    if was_training:
        model.train()
    return float(ret.mean()), float(ret.std()), float(torch.where(red_b, final > 0, final < 0).double().mean())


# ---- Matches: any two sides against each other, each with its own eyes, with the device episode statistics ------------------------
MATCH_BOTS = ("random", "baseline", "approxq")


class MatchSide:
    """One side of play_match: a network (`model`, a MAPPOAgent) or an in-kernel team (`bot` out of MATCH_BOTS).  greedy / mask_illegal:
    how a network picks its actions (argmax in place of a draw; over the legal actions only).  fog_of_war, sight_range, belief,
    belief_weights, belief_evidence: the observation regime the network was trained under, with evaluate_vectorized's meaning and
    dependencies.  A bot side takes none of them (play_match's fog_bots binds the bots to the opponent's sight rule)."""

    def __init__(self, model=None, bot=None, greedy=False, mask_illegal=False, fog_of_war=False, sight_range=SIGHT_RANGE, belief=False,
                 belief_weights=False, belief_evidence=False):
        if (model is None) == (bot is None):
            raise ValueError("a MatchSide is either a network (model=...) or an in-kernel team (bot=...), exactly one of the two")
        if bot is not None and bot not in MATCH_BOTS:
            raise ValueError(f"bot must be one of {MATCH_BOTS}, got {bot!r}")
        if bot is not None and (greedy or mask_illegal or fog_of_war or belief or belief_weights or belief_evidence):
            raise ValueError("a bot side takes no policy or observation flags (fog_bots=True of play_match binds the bots to the sight rule)")
        if belief and not fog_of_war:
            raise ValueError("belief=True needs fog_of_war=True")
        if belief_weights and not (fog_of_war and belief):
            raise ValueError("belief_weights=True needs fog_of_war=True and belief=True")
        if belief_evidence and not (fog_of_war and belief):
            raise ValueError("belief_evidence=True needs fog_of_war=True and belief=True")
        if fog_of_war and not 0 <= int(sight_range) <= _lib.SIGHT_RANGE_MAX:
            raise ValueError(f"sight_range must be in 0 .. {_lib.SIGHT_RANGE_MAX}, got {sight_range!r}")
        self.model, self.bot, self.greedy, self.mask_illegal = model, bot, bool(greedy), bool(mask_illegal)
        self.fog_of_war, self.sight_range = bool(fog_of_war), int(sight_range)
        self.belief, self.belief_weights, self.belief_evidence = bool(belief), bool(belief_weights), bool(belief_evidence)


def match_side_seed(seed, k):
    """The seed of side k's action draws (k = 0 for A, 1 for B): 2 * seed + k in 32 bits, so the two sides of one match and the sides
    of matches with neighbouring seeds all draw from different streams (pmx_policy_sample hashes seed, row and tick together)."""
    return ((int(seed) << 1) | int(k)) & 0xFFFFFFFF


def match_colours(n_envs, colours, device="cpu"):
    """uint8 [n_envs], non-zero = side A is red in that env: "both" = red in envs [0, n_envs // 2) and blue in the rest (the split
    of evaluate_vectorized(side="both")), "red" / "blue" = that colour everywhere."""
    if colours not in ("both", "red", "blue"):
        raise ValueError(f"colours must be both, red or blue, got {colours!r}")
    red = torch.zeros(n_envs, dtype=torch.uint8, device=device)
    red[:{"red": n_envs, "both": n_envs // 2, "blue": 0}[colours]] = 1
    return red


def _check_match(a, b, fog_bots):
    for s in (a, b):
        if not isinstance(s, MatchSide):
            raise ValueError(f"play_match takes two MatchSide objects, got {type(s).__name__}")
    if a.model is not None and b.model is not None and a.greedy and b.greedy:
        raise ValueError("two greedy networks and no bot make every game of a colour the same game: let at least one side sample "
                         "(greedy=False), or this would play n_envs copies of two games")
    if fog_bots:
        ranges = [o.sight_range for s, o in ((a, b), (b, a)) if s.bot is not None and o.fog_of_war and o.sight_range >= 1]
        if not ranges:
            raise ValueError("fog_bots=True needs a bot side whose opponent has fog_of_war=True and sight_range >= 1")
        return ranges[0]
    return None


def match_result(red, score, ret_a, ret_b, stats):
    """play_match's bookkeeping from its raw tensors: red uint8 [n] (A's colour), score int32 [n] (final data.score), ret_a / ret_b
    float64 [n] (each side's summed team reward), stats int32 [48, n].  -> the result dict (see play_match)."""
    n = int(red.shape[0])
    red_b = red.to(torch.bool)
    margin = torch.where(red_b, score, -score).to(torch.float64)             # A's signed final score
    per = stats[:32].view(4, 8, n).to(torch.float64)                         # [agent, counter, game]

    def split(mask):
        g = int(mask.sum())
        if g == 0:
            return dict(games=0)
        m = margin[mask]
        return dict(games=g, wins_a=int((m > 0).sum()), ties=int((m == 0).sum()), wins_b=int((m < 0).sum()),
                    win_rate_a=float((m > 0).double().mean()), margin_mean=float(m.mean()),
                    margin_sem=float(m.std() / g ** 0.5) if g > 1 else 0.0)

    def side(team_red):
        # the side's two slots, lower agent index first (the offensive bot of an in-kernel team): agents (0, 2) where it is red
        first = torch.where(team_red, per[0], per[1])
        second = torch.where(team_red, per[2], per[3])
        return {name: [float(first[c].mean()), float(second[c].mean())] for c, name in enumerate(_lib.STAT_NAMES)}

    out = split(torch.ones_like(red_b))
    out.update(as_red=split(red_b), as_blue=split(~red_b), ticks_mean=float(stats[_lib.STATS_W_TICKS].double().mean()),
               return_a=float(ret_a.mean()), return_b=float(ret_b.mean()), stats_a=side(red_b), stats_b=side(~red_b), red=red, score=score, stats=stats)
    return out


class _MatchEyes:
    """What one network side of a match owns: its colour vector, observation buffer and belief buffers, and the three calls of a tick."""

    def __init__(self, side, env, red, seed, autocast):
        self.side, self.env, self.red, self.seed = side, env, red, seed
        n = env.n_envs
        dev = red.device
        self.obs = torch.empty((n, 2) + tuple(env.obs_shape), dtype=env.obs_torch_dtype, device=dev)
        self.ctx = torch.autocast(device_type=dev.type, dtype=torch.bfloat16) if autocast else _NullCtx()
        self.kw = {"sight_range": side.sight_range} if side.fog_of_war else {}
        self.bel = self.wts = self.lev = None
        if side.belief_weights:
            self.bel, self.wts, self.lev = env.belief_weights_init(env.new_belief(), *env.new_belief_weights(), 0)
            self.kw = {"levels": self.lev}
        elif side.belief:
            self.bel = env.belief_init(env.new_belief(), 0)
            self.kw = {"belief": self.bel}
        self.ekw = {"evidence": env.belief_evidence_init(env.new_belief_evidence())} if side.belief_evidence else {}

    def act(self, tick):
        """this tick's two actions per env, in the env's frame: int64 [n, 2]"""
        env, side = self.env, self.side
        env.emit_team_obs_mixed(self.red, self.obs, **self.kw)
        lo = self.obs.view((-1,) + tuple(env.obs_shape))
        lg = mappo.canonicalize_legal(mappo.team_columns(env.legal, self.red), self.red).reshape(-1) if side.mask_illegal else None
        with self.ctx:
            if side.greedy:          # the very call evaluate_vectorized makes (torch's argmax without masks, the kernel's with them)
                a = side.model.get_deterministic_action(lo, **({"legal": lg} if lg is not None else {}))
            else:
                a = mappo.sample_actions(side.model.logits(lo), lg, seed=self.seed, counter=tick, greedy=False)[0]
        return mappo.canonicalize_action(a.view(-1, 2), self.red)

    def after_step(self):
        if self.side.belief_weights:
            self.env.belief_weights_update(self.red, self.bel, self.wts, self.lev, self.side.sight_range, **self.ekw)
        elif self.side.belief:
            self.env.belief_update(self.red, self.bel, self.side.sight_range, **self.ekw)


@torch.no_grad()
def play_match(a, b, layout="bloxCapture", n_envs=1024, length=300, colours="both", device="cuda:0", seed=0, autocast=True, fog_bots=False,
               env=None, record=0):
    """n_envs games at once between two MatchSides, each seeing the game its own way, with the device episode statistics
    (pmx_episode_stats_update) of every game.  colours: see match_colours; B's colours are A's inverted.  Per tick every network side
    gets one pmx_emit_team_obs_mixed* call of its own regime and colours, runs its own forward, and draws with
    mappo.sample_actions(seed=match_side_seed(seed, k), counter=tick) -- or, greedy, takes evaluate_vectorized's argmax; a bot side
    writes its two action codes.  After the step each side's belief buffers advance under its own colours.  The env never resets
    (auto_reset=False): a game counts up to its first done, and the loop ends when every game is DONE or after length + 1 ticks.
    fog_bots: the in-kernel bots obey the sight rule at the opposing network's sight_range (pmx_set_bot_sight).
    Returns a dict: games, wins_a / ties / wins_b, win_rate_a, margin_mean / margin_sem (A's signed final score, +score where A is
    red), the same under as_red / as_blue, ticks_mean, return_a (mean over games of A's summed team reward, as evaluate_vectorized sums
    it), stats_a / stats_b (per counter of _lib.STAT_NAMES the per-game means of the side's two slots, lower agent index first), and
    the raw tensors red [n], score [n], stats [48, n].
    record=k: the first min(k, n_envs) games are logged sub-step by sub-step (pmx_game_record_update) and the result's "record" is
    their game_record.GameRecord (meta: A's colour per game, the sides' names); 0: no log, no extra call, "record" is None.
    Two greedy networks are refused (every game of a colour would be the same game).  `env`: a ready env in place of the PmxVecEnv
    this function creates (tests)."""
    bot_sight = _check_match(a, b, fog_bots)
    dev = torch.device(device)
    red_a = match_colours(n_envs, colours, dev)
    reds = (red_a, 1 - red_a)
    if env is None:
        env = PmxVecEnv(layout, n_envs, length=length, auto_reset=False, obs_dtype="bfloat16" if autocast else "float32", device=dev,
                        seed=seed, bots=any(s.bot in BOT_TEAMS for s in (a, b)))
    if bot_sight is not None:
        env.set_bot_sight(bot_sight)
    env.reset(want_obs=False)
    stats = env.episode_stats_init(env.new_episode_stats())
    record = max(0, min(int(record), n_envs))
    rec = env.game_record_init(env.new_game_record(0, record)) if record else None
    models = [s.model for s in (a, b) if s.model is not None]
    was_training = [m.training for m in models]
    for m in models:
        m.eval()
    acts = torch.empty((n_envs, 4), dtype=torch.int8, device=dev)
    eyes = []
    for k, s in enumerate((a, b)):
        if s.model is not None:
            eyes.append(_MatchEyes(s, env, reds[k], match_side_seed(seed, k), autocast))
        else:
            codes = BOT_TEAMS.get(s.bot, (_lib.ACTION_RANDOM_LEGAL,) * 2)
            mappo.set_team_columns(acts, reds[k], torch.tensor(codes, dtype=torch.int8, device=dev)[None].expand(n_envs, 2))
    red_b = red_a.to(torch.bool)
    alive = torch.ones(n_envs, dtype=torch.bool, device=dev)
    ret = torch.zeros(n_envs, dtype=torch.float64, device=dev)
    ret_b = torch.zeros(n_envs, dtype=torch.float64, device=dev)
    final = torch.zeros(n_envs, dtype=torch.int32, device=dev)
    for tick in range(length + 1):
        for e in eyes:
            mappo.set_team_columns(acts, e.red, e.act(tick))
        _, rew, done, info = env.step(acts, want_obs=False)
        for e in eyes:
            e.after_step()
        env.episode_stats_update(stats, done)
        if rec is not None:
            env.game_record_update(rec, done)
        own = torch.where(red_b, rew[:, 0], rew[:, 1])
        ret += torch.where(alive, own + own, torch.zeros_like(ret))                 # sum over both of A's agents' rewards (:328)
        other = torch.where(red_b, rew[:, 1], rew[:, 0])
        ret_b += torch.where(alive, other + other, torch.zeros_like(ret_b))
        d = done.to(torch.bool) & alive
        final = torch.where(d, info["score"], final)
        alive &= ~d
        if not bool(alive.any()):
            break
    env.close()
    for m, t in zip(models, was_training):
        if t:
            m.train()
    R = stats[8 * 0 + _lib.STAT_RETURNED] + stats[8 * 2 + _lib.STAT_RETURNED] - stats[8 * 1 + _lib.STAT_RETURNED] - stats[8 * 3 + _lib.STAT_RETURNED]
    if not bool((stats[_lib.STATS_W_DONE] == 1).all()):
        raise RuntimeError(f"play_match: {int((stats[_lib.STATS_W_DONE] != 1).sum())} games are not DONE after {length + 1} ticks")
    if not torch.equal(stats[_lib.STATS_W_SCORE], final):
        raise RuntimeError("play_match: the statistics' SCORE differs from the score the env reported at a game's done")
    if not torch.equal(R, final):
        raise RuntimeError("play_match: red RETURNED minus blue RETURNED differs from the final score")
    out = match_result(red_a, final, ret, ret_b, stats)
    out["record"] = None
    if rec is not None:
        names = [s.bot if s.model is None else "network" for s in (a, b)]
        out["record"] = rec.to_host(a_is_red=[int(v) for v in red_a[:record].tolist()], side_a=str(names[0]), side_b=str(names[1]), seed=int(seed))
    return out


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
