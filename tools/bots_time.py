"""Rule / expansion kernel time per tick at 16 384 smallCapture envs, by what plays red (default), or with --bot-sight N the
rule kernel with baselineTeam on BOTH sides, bot sight off / N / off again in one process (pmx_set_bot_sight)."""
import argparse, sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N = 16384


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bot-sight", type=int, default=None, help="time the rule kernel with baselineTeam bots on BOTH sides, bot sight off / N / off "
                    "again in one process (pmx_set_bot_sight), --ticks profiled ticks per arm, and nothing else")
    ap.add_argument("--ticks", type=int, default=500)
    return ap


def sight_arms(sight, ticks):
    import torch, pmx
    env = pmx.PmxVecEnv("smallCapture", N, length=300, auto_reset=True, obs_dtype="uint8", bots=True)
    act = torch.empty((N, 4), dtype=torch.int8, device="cuda")
    act[:, 0], act[:, 1], act[:, 2], act[:, 3] = -3, -3, -4, -4
    for arm, s in (("off", None), (f"sight {sight}", sight), ("off again", None)):
        env.set_bot_sight(s)
        env.reset()                                  # every arm starts from fresh games
        for _ in range(20): env.step(act)
        env.profile_begin(ticks + 20)
        for _ in range(ticks): env.step(act)
        p = env.profile_end()
        print(json.dumps({"arm": arm, "actions": "baselineTeam on both sides", "ticks": ticks, "rule_us": p["rule_ms"] / p["rule_launches"] * 1e3,
                          "expand_us": p["expand_ms"] / p["expand_launches"] * 1e3}), flush=True)
    env.close()


def red_variants():
    import torch, pmx
    for bots in (False, True):
        env = pmx.PmxVecEnv("smallCapture", N, length=300, auto_reset=True, obs_dtype="uint8", bots=bots)
        env.reset()
        g = torch.Generator(device="cuda").manual_seed(0)
        a = torch.randint(0, 5, (N, 4), generator=g, device="cuda", dtype=torch.int8)
        variants = {"random actions": a}
        if bots:
            b = a.clone(); b[:, 0] = -3; b[:, 2] = -4
            variants["red = baselineTeam (offense, defense)"] = b
            c = a.clone(); c[:, 0] = -2; c[:, 2] = -2
            variants["red = randomTeam in-kernel"] = c
            d = a.clone(); d[:, 0] = -5; d[:, 2] = -6
            variants["red = approxQTeam (offense, defense)"] = d
        for name, act in variants.items():
            for _ in range(20): env.step(act)
            env.profile_begin(220)
            for _ in range(200): env.step(act)
            p = env.profile_end()
            print(json.dumps({"bots_handle": bots, "actions": name, "rule_us": p["rule_ms"] / p["rule_launches"] * 1e3, "expand_us": p["expand_ms"] / p["expand_launches"] * 1e3}))
        env.close()


def main():
    args = parser().parse_args()
    if args.bot_sight is not None:
        sight_arms(args.bot_sight, args.ticks)
    else:
        red_variants()


if __name__ == "__main__":
    main()
