"""Print a saved game record (tools/match.py --record, GameRecord.save): boards as text, or the event list.  Uses no GPU.

    python tools/replay.py games.npz                          every tick of game 0, the board after the tick's fourth sub-step
    python tools/replay.py games.npz --game 2 --from 40 --to 60 --substeps
    python tools/replay.py games.npz --events                 one line per sub-step in which something happened
"""
import argparse
import importlib.util
import os
import sys

# game_record.py is plain numpy: it is loaded by path, so that reading a record needs neither torch nor the HIP library
_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pacman-marl-2025_amd", "game_record.py")
_spec = importlib.util.spec_from_file_location("pmx_game_record", _PATH)
game_record = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(game_record)


def event_line(ev):
    tick, mover, move, died, victims, ate, capsule, returned = ev
    what = [f"agent {mover} {game_record.MOVE_NAMES[move]}"]
    if ate:
        what.append("eats a pellet")
    if capsule:
        what.append("eats a capsule")
    if returned:
        what.append(f"returns {returned}")
    if died:
        what.append("dies")
    what += [f"kills agent {v}" for v in victims]
    return f"tick {tick:4d}.{mover}  " + ", ".join(what)


def main(argv=None, out=sys.stdout):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("path")
    ap.add_argument("--game", type=int, default=0)
    ap.add_argument("--from", dest="first", type=int, default=0, help="first tick")
    ap.add_argument("--to", dest="last", type=int, default=None, help="last tick (default: the game's last)")
    ap.add_argument("--substeps", action="store_true", help="a board after every sub-step, not only after the tick")
    ap.add_argument("--events", action="store_true", help="the event list in place of the boards (every move with --substeps)")
    args = ap.parse_args(argv)
    rec = game_record.GameRecord.load(args.path)
    g = args.game
    if not 0 <= g < rec.games:
        ap.error(f"--game {g}: the record holds games 0 .. {rec.games - 1}")
    n = rec.length(g)
    last = n - 1 if args.last is None else min(args.last, n - 1)
    print(f"game {g} of {rec.games}: {n} ticks, final score {rec.final_score(g)}" + (", done" if rec.done(g) else "")
          + (", log full" if rec.overflow(g) else "") + (f"  {rec.meta}" if rec.meta else ""), file=out)
    if args.events:
        for ev in rec.events(g):
            quiet = not (ev[3] or ev[4] or ev[5] or ev[6] or ev[7])
            if args.first <= ev[0] <= last and (args.substeps or not quiet):
                print(event_line(ev), file=out)
        return 0
    if args.first == 0:
        print("start", file=out)
        print(rec.render(g, -1), end="", file=out)
    events = rec.events(g)
    for t in range(args.first, last + 1):
        for m in (range(4) if args.substeps else (3,)):
            print(f"tick {t}.{m}" if args.substeps else f"tick {t}", file=out)
            print(rec.render(g, t, m), end="", file=out)
            for ev in events[4 * t + (m if args.substeps else 0):4 * t + m + 1]:
                if ev[3] or ev[4] or ev[5] or ev[6] or ev[7]:
                    print(event_line(ev), file=out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
