"""Head-to-head match between two sides (pmx.trainer.play_match): prints one JSON line.

A side is an EMA checkpoint (tools/train.py --save) or the name of an in-kernel team (random, baseline, approxq).  The flags of
tools/train.py that shape a policy's inputs are given per side, with the prefix --a- / --b-: each network sees the game under the
regime it was trained with.

    python tools/match.py fog.pt belief.pt --a-fog-of-war --b-fog-of-war --b-belief --games 1024 --layout smallCapture
    python tools/match.py ckpt.pt baseline --a-greedy
    python tools/match.py approxq baseline
    python tools/match.py approxq baseline --record games.npz --record-games 8        (then: python tools/replay.py games.npz --events)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import pmx
from pmx import mappo, trainer

SIDE_FLAGS = ("greedy", "mask_illegal", "fog_of_war", "belief", "belief_weights", "belief_evidence")


def add_side_flags(ap, k):
    for f in SIDE_FLAGS:
        ap.add_argument(f"--{k}-{f.replace('_', '-')}", action="store_true", help=f"side {k.upper()}: MatchSide({f}=True)")
    ap.add_argument(f"--{k}-sight-range", type=int, default=trainer.SIGHT_RANGE, help=f"side {k.upper()}: with --{k}-fog-of-war, Manhattan cells")


def make_side(args, k, what, layout, device):
    if what in trainer.MATCH_BOTS:
        return trainer.MatchSide(bot=what)
    lay = pmx.get_layout(layout)
    model = mappo.MAPPOAgent((8, lay.height, lay.width), 5, 2).to(device)
    model.load_state_dict(torch.load(what, map_location=device, weights_only=True))
    return trainer.MatchSide(model=model, sight_range=getattr(args, f"{k}_sight_range"), **{f: getattr(args, f"{k}_{f}") for f in SIDE_FLAGS})


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a", help="side A: an EMA checkpoint, or one of " + ", ".join(trainer.MATCH_BOTS))
    ap.add_argument("b", help="side B, likewise")
    add_side_flags(ap, "a")
    add_side_flags(ap, "b")
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--layout", default="smallCapture")
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--colours", default="both", choices=["both", "red", "blue"], help="side A's colour (both: red in the first half of the games)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fog-bots", action="store_true", help="a bot side obeys the sight rule of the opposing network (needs that side's fog-of-war)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--record", metavar="PATH", help="save a game record (.npz) of the first --record-games games; tools/replay.py prints it")
    ap.add_argument("--record-games", type=int, default=4, help="with --record: how many games to log")
    args = ap.parse_args(argv)
    sides = [make_side(args, k, what, args.layout, args.device) for k, what in (("a", args.a), ("b", args.b))]
    r = trainer.play_match(sides[0], sides[1], layout=args.layout, n_envs=args.games, length=args.length, colours=args.colours,
                           device=args.device, seed=args.seed, fog_bots=args.fog_bots, record=args.record_games if args.record else 0)
    record = r.pop("record", None)
    out = {k: v for k, v in r.items() if not isinstance(v, torch.Tensor)}
    if record is not None:
        record.meta.update(a=args.a, b=args.b, layout=args.layout)
        record.save(args.record)
        out.update(record=args.record, record_games=record.games)
    out.update(a=args.a, b=args.b, layout=args.layout, colours=args.colours, seed=args.seed)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
