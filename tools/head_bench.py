#!/usr/bin/env python3
"""Times the first actor-head layer, Linear(32 H W -> 512), both ways: the library path MAPPOAgent.logits keeps with fused_head off
(a permuted copy of the bfloat16 shadow weight + F.linear, autograd's backward) against actor_head._ActorHead (csrc/pmx_actor_head.hip:
pack + products), in ONE process with the arms alternating, on device events.  The library arm is timed twice (lib_a, lib_b) so that
its own run-to-run spread stands beside every comparison.  The entry points of the new kernels are also timed alone through the C ABI
(pack, forward, backward = the input-gradient and the weight/bias-gradient products together).
    python tools/head_bench.py [--calls 200] [--out FILE]"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("smallCapture", 11, 14, 512, True), ("smallCapture", 11, 14, 1024, True), ("smallCapture", 11, 14, 2048, True),
          ("smallCapture", 11, 14, 4096, True), ("smallCapture", 11, 14, 16384, True),
          ("smallCapture", 11, 14, 32768, False),          # the rollout's inference batch: forward only
          ("bloxCapture", 20, 20, 512, True), ("bloxCapture", 20, 20, 2048, True), ("bloxCapture", 20, 20, 8192, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="timed calls per arm (in rounds of 20, the arms alternating)")
    ap.add_argument("--out", default="", help="also write the lines to this file")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from pmx import _lib, actor_head
    lib = _lib.load()
    dev = torch.device("cuda")
    per_round = 20
    rounds = max(1, (args.calls + per_round - 1) // per_round)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def time_arms(arms):
        """arms: {name: fn} -> {name: microseconds per call}, the arms taking turns round by round"""
        for fn in arms.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        total = {k: 0.0 for k in arms}
        for _ in range(rounds):
            for k, fn in arms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(per_round):
                    fn()
                b.record()
                b.synchronize()
                total[k] += a.elapsed_time(b)
        return {k: 1e3 * v / (rounds * per_round) for k, v in total.items()}

    for label, H, W, B, train in SHAPES:
        HW, K = H * W, 32 * H * W
        flop = 2.0 * B * K * 512
        torch.manual_seed(0)
        feat = torch.randn(B, HW, 32, device=dev).to(torch.bfloat16).requires_grad_(True)
        w32 = (0.02 * torch.randn(512, K, device=dev)).requires_grad_(True)
        b32 = (0.1 * torch.randn(512, device=dev)).requires_grad_(True)
        w16, b16 = w32.detach().to(torch.bfloat16).requires_grad_(True), b32.detach().to(torch.bfloat16).requires_grad_(True)
        dh = torch.randn(B, 512, device=dev).to(torch.bfloat16)

        def lib_fwd():
            w = w16.view(512, 32, HW).permute(0, 2, 1).reshape(512, K)
            return F.linear(feat.reshape(B, K), w, b16)

        def new_fwd():
            return actor_head._ActorHead.apply(feat, w32, b32, H, W, None)

        def lib_fb():
            return torch.autograd.grad(lib_fwd(), [feat, w16, b16], dh)

        def new_fb():
            return torch.autograd.grad(new_fwd(), [feat, w32, b32], dh)

        def no_grad(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            t = time_arms({"lib_a": no_grad(lib_fwd), "new": no_grad(new_fwd), "lib_b": no_grad(lib_fwd)})
            emit({"shape": label, "H": H, "W": W, "B": B, "what": "forward", "us": t, "tflops": {k: flop / v * 1e-6 for k, v in t.items()}})
            if train:
                t = time_arms({"lib_a": lib_fb, "new": new_fb, "lib_b": lib_fb})
                emit({"shape": label, "H": H, "W": W, "B": B, "what": "forward+backward", "us": t,
                      "tflops": {k: 3 * flop / v * 1e-6 for k, v in t.items()}})
        # the entry points alone
        pk, sc = actor_head.actor_head_sizes(H, W, B)
        pack = torch.empty(pk, dtype=torch.uint8, device=dev)
        scratch = torch.empty(sc, dtype=torch.uint8, device=dev)
        h = torch.empty(B, 512, dtype=torch.bfloat16, device=dev)
        fd, wd, bd = feat.detach(), w32.detach(), b32.detach()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        arms = {"pack": lambda: _lib.check(lib.pmx_actor_head_pack(wd.data_ptr(), pack.data_ptr(), H, W, st)),
                "forward": lambda: _lib.check(lib.pmx_actor_head_forward(fd.data_ptr(), pack.data_ptr(), bd.data_ptr(), h.data_ptr(), scratch.data_ptr(),
                                                                         B, H, W, st))}
        if train:
            dfeat = torch.empty_like(fd)
            dw, db = torch.empty(512, K, device=dev), torch.empty(512, device=dev)
            arms["backward"] = lambda: _lib.check(lib.pmx_actor_head_backward(fd.data_ptr(), dh.data_ptr(), pack.data_ptr(), dfeat.data_ptr(), dw.data_ptr(),
                                                                              db.data_ptr(), scratch.data_ptr(), B, H, W, st))
        t = time_arms(arms)
        prod = {"pack": 0, "forward": 1, "backward": 2}
        emit({"shape": label, "H": H, "W": W, "B": B, "what": "entry points alone", "us": t,
              "tflops": {k: prod[k] * flop / v * 1e-6 for k, v in t.items() if prod[k]}})
        del feat, w32, b32, w16, b16, dh, pack, scratch, h
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
