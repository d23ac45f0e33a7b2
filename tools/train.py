#!/usr/bin/env python3
"""MAPPO training on the vectorised env, one process per GPU.

    python tools/train.py --envs 16384 --horizon 32 --updates 100
    python tools/train.py --layout mazes --maze-size 32x16 --envs 4096 ...      (BASELINE config 5's boards)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 tools/train.py --envs 8192 ...

Every rank owns its env shard, rollout buffers, GAE and minibatch sampling; the only exchange is one flat-gradient
all-reduce per optimizer step over RCCL (pmx.mappo.PPOLearner)."""
import argparse, json, os, sys, time
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")    # before HIP initialises: see pacman-marl-2025_amd/__init__.py
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def maze_size(text):
    """'WxH' -> (W, H) of a board the maze generator can produce (a mirrored half of (W - 2) / 2 columns inside a wall frame)."""
    try:
        w, h = (int(v) for v in text.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError("expected WxH, e.g. 32x16")
    if w % 2 or not 8 <= w <= 32 or not 3 <= h <= 32:
        raise argparse.ArgumentTypeError("maze boards are 8..32 wide (even) and 3..32 high")
    return w, h


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", default="smallCapture", help='a layout name, or "mazes": one distinct generated maze per env (BASELINE config 5)')
    ap.add_argument("--maze-size", type=maze_size, default=(20, 20), metavar="WxH",
                    help="with --layout mazes: the generated boards' size (default 20x20; BASELINE config 5 names 32x16)")
    ap.add_argument("--redraw", action="store_true", help="with --layout mazes: every reset moves the env to a freshly drawn maze of the pool "
                                                          "(the reference's random_layout=True, gymPacMan.py:98-100)")
    ap.add_argument("--log", default="", help="append the per-update JSON lines to this file as well (tools/plot_log.py plots it)")
    ap.add_argument("--envs", type=int, default=16384, help="envs per GPU")
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--minibatch", type=int, default=8192, help="samples per optimizer step per GPU (reference: 512)")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--total-updates", type=int, default=2000)
    ap.add_argument("--opponent", default="curriculum", choices=["random", "baseline", "approxq", "self", "pool", "curriculum"])
    ap.add_argument("--hard-bots", default="baseline", help="comma-separated in-kernel teams the curriculum draws its hard opponent from (baseline, approxq)")
    ap.add_argument("--obs", default=None, choices=["float32", "bfloat16", "uint8"], help="observation planes; default: the trainer's choice (uint8 under bf16 autocast, float32 otherwise)")
    ap.add_argument("--algorithm", default="mappo", choices=["mappo", "ippo"])
    ap.add_argument("--eval-every", type=int, default=0)
    ap.add_argument("--save", default="")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--unpaired", action="store_true", help="the reference's independent shuffle of agent samples (critic runs per sample)")
    ap.add_argument("--curriculum-scale", type=float, default=1.0, help="compress the curriculum's phase thresholds (updates 200 / 800)")
    ap.add_argument("--mask-illegal", action="store_true", help="sample, train and evaluate over the legal actions only (the env's legal-action masks; "
                                                                "off by default: the reference samples from all five logits)")
    ap.add_argument("--mix-opponents", action="store_true", help="spread the opponent mixture over the envs of every rollout (self / pool / bots side by side, "
                                                                 "both colours) instead of one opponent and one colour per rollout")
    ap.add_argument("--eval-side", default="blue", choices=["blue", "red", "both"], help="the colour the evaluated policy plays (both: red in the first half of "
                                                                                         "the envs); a policy trained with --mix-opponents plays both")
    ap.add_argument("--fog-of-war", action="store_true", help="the contest's sight rule on every policy input: an enemy shows only within --sight-range of one of the "
                                                              "team's two agents (the critic's merged input stays full); the evaluation runs under the same rule")
    ap.add_argument("--belief", action="store_true", help="with --fog-of-war: track, per hidden enemy, the set of cells it can be on (sight rule, noisy sonar "
                    "distances, motion) on the device and show the sets in plane 5 of every policy input, in training and in the evaluations")
    ap.add_argument("--belief-weights", action="store_true", help="with --fog-of-war --belief: refine the sets by an exact Bayes filter on the device (random-walk "
                    "motion, respawn prior, sight rule, sonar) and show its levels 0 .. 16 in plane 5 in place of the sets' 0 / 1")
    ap.add_argument("--belief-evidence", action="store_true", help="with --fog-of-war --belief: narrow the sets by what stays public about a hidden enemy: "
                    "the half it is on, a pellet it ate, and that it can only have died next to one of the team's agents")
    ap.add_argument("--fog-bots", action="store_true", help="with --fog-of-war: the in-kernel bot opponents obey the sight rule too (an enemy counts only "
                    "within --sight-range of the bot or its mate, as the contest hands its bots an observation); training and the evaluations")
    ap.add_argument("--sight-range", type=int, default=5, help="with --fog-of-war: Manhattan cells (the contest's SIGHT_RANGE is 5)")
    ap.add_argument("--graph", action="store_true", help="replay the optimizer step from a hipGraph (launch-bound minibatches, e.g. 512)")
    return ap


def layouts(args, rank=0):
    """The trainer's `layout` argument: the name, or for "mazes" one generated maze of --maze-size per env -- the reference
    generator's seeds, a disjoint range per rank."""
    if args.layout != "mazes":
        return args.layout
    from pmx import maze_generator
    from pmx.layout import Layout
    w, h = args.maze_size
    return [Layout.from_text(maze_generator.generate_maze(s, rows=h - 2, cols=(w - 2) // 2))
            for s in range(rank * args.envs + 1, (rank + 1) * args.envs + 1)]


def main():
    args = parser().parse_args()

    rank, world, local = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local)
    pg = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    from pmx import trainer

    layout = layouts(args, rank)
    eval_layout = layout[:1024] if isinstance(layout, list) else layout

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.log:
            with open(args.log, "a") as fh:
                fh.write(line + "\n")

    fog = {"fog_of_war": True, "sight_range": args.sight_range} if args.fog_of_war else {}
    if args.belief:
        fog["belief"] = True                                    # (without --fog-of-war the trainer rejects it)
    if args.belief_weights:
        fog["belief_weights"] = True                            # (without --belief the trainer rejects it)
    if args.belief_evidence:
        fog["belief_evidence"] = True                           # (likewise)
    if args.fog_bots:
        fog["fog_bots"] = True                                  # (without --fog-of-war the trainer rejects it)
    tr = trainer.VecMAPPOTrainer(layout, args.envs, horizon=args.horizon, minibatch=args.minibatch, epochs=args.epochs, redraw_layouts=args.redraw,
                                 obs_dtype=args.obs, device=f"cuda:{local}", seed=args.seed, rank=rank, world_size=world,
                                 total_updates=args.total_updates, opponent=args.opponent, algorithm=args.algorithm, use_graph=args.graph, paired_minibatches=not args.unpaired, curriculum_scale=args.curriculum_scale,
                                 hard_bots=tuple(args.hard_bots.split(",")), mask_illegal=args.mask_illegal,
                                 **({"mix_opponents": True} if args.mix_opponents else {}), **fog)
    for u in range(args.updates):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        st = tr.train_update()
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        if rank == 0:
            f = lambda k: float(st[k]) if k in st else None
            by_mode = {"by_mode": {m: [int(st["episodes_by_mode"][m]), int(st["wins_by_mode"][m])] for m in st["episodes_by_mode"]}} if args.mix_opponents else {}
            emit(dict(update=u, algorithm=args.algorithm, opponent=st["opponent"], red=st["play_as_red"], sec=round(dt, 3),
                                  env_steps_per_s=round(world * tr.N * tr.T / dt), episodes=int(st["episodes"]),
                                  win_rate=(float(st["wins"]) / max(int(st["episodes"]), 1)),
                                  reward=float(st["rollout_reward"]) / max(tr.N, 1), pg=f("pg"), vl=f("vl"), entropy=f("entropy"),
                                  clip_frac=f("clip_frac"), grad_norm=f("grad_norm"), steps=st["optimizer_steps"], **by_mode))
            if args.eval_every and u and u % args.eval_every == 0:
                emit(dict(update=u, algorithm=args.algorithm,
                          eval_vs_baseline=trainer.evaluate_vectorized(tr.model, eval_layout, 1024, "baseline", device=f"cuda:{local}", mask_illegal=args.mask_illegal, side=args.eval_side, **fog),
                          eval_vs_random=trainer.evaluate_vectorized(tr.model, eval_layout, 1024, "random", device=f"cuda:{local}", mask_illegal=args.mask_illegal, side=args.eval_side, **fog)))
    if rank == 0 and args.save:
        tr.save_ema(args.save)
    if world > 1:
        dist.barrier(); dist.destroy_process_group()


if __name__ == "__main__":
    main()
