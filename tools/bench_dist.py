"""Cost of Gaussian distributional Q-learning in one process: alternating timed windows of TD updates at batch B (bf16) through four
steppers.  The key on against off: `dqn`, a TDStepper with distributional=False, and `dist`, one with distributional=True, on the
same spread-head engine (as tools/bench_iql.py alternates its variants).  The head against no head: `plain`, a TDStepper on an
engine without the spread head (the parent's update, launch for launch), and `spread`, the same stepper on a spread-head engine of
its own, whose Q layer's GEMM has 30 live output rows where the plain one has 15.  Then the device time of the loss launch of each
(launch profiler, windows of their own).  The three forward passes and the backward keep their shapes, so the expected difference
between `dqn` and `dist` is the loss launch alone, and between `plain` and `spread` the Q layer's thin GEMMs.

Read the second pair with care: in a process that holds several steppers, those created after the first have been measured up to
a quarter slower than the first whatever engine they run on (two plain steppers on a plain engine included), so `spread` against
`plain` shows the position in the process, not the head; profiles/dist_record.txt has the figures of engines measured one at a
time.  `dqn` and `dist` sit side by side and share every buffer of the engine, which is why that pair is the one to trust.

    python tools/bench_dist.py [--batch 256] [--steps 30] [--rounds 6] [--out profiles/dist_bench.json]

The baseline is never a separate run: two processes differ by more than the effect looked for."""
import argparse
import json
import os
import sys
import time

import torch

KERNELS = ("td_loss", "td_loss_dist")


def _median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--pool", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from video_dqn_amd import _lib, synth
    from video_dqn_amd.engine import NetEngine, TDStepper
    dev = "cuda"
    B = args.batch
    plain = NetEngine(3, 5, 1, True, "bf16", 2 * B, device=dev)
    plain.load_tensors(synth.make_state_dict(7))

    def spread_engine():
        net = NetEngine(3, 5, 1, True, "bf16", 2 * B, device=dev, spread_head=True)
        net.load_tensors(synth.make_state_dict(7))
        g = torch.Generator().manual_seed(3)
        net.view("spread.weight").copy_((torch.rand(15, 256, generator=g) * 2 - 1) / 16)
        net.view("spread.bias").copy_((torch.rand(15, generator=g) * 2 - 1) / 16)
        net.mark_dirty()
        return net

    net, alone = spread_engine(), spread_engine()
    kw = dict(lr=1e-4, gamma=0.99, clip_rect=True)
    steppers = {"plain": TDStepper(plain, B, **kw),
                "spread": TDStepper(alone, B, **kw),
                "dqn": TDStepper(net, B, distributional=False, **kw),
                "dist": TDStepper(net, B, distributional=True, **kw)}
    (tup, raw) = synth.make_batch(5, args.pool, 1, structured=True, reward_p=0.05)
    before = torch.from_numpy(raw[0]).to(dev)
    after = torch.from_numpy(raw[1]).to(dev)
    act, rew, term = tup[2].to(dev), tup[3].float().to(dev), tup[4].float().to(dev)
    idxs = [torch.randint(0, args.pool, (B,), device=dev) for _ in range(16)]
    modes = list(steppers)
    k = [0]

    def window(mode, steps):
        stp = steppers[mode]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            k[0] += 1
            idx = idxs[k[0] % 16]
            stp.step(before[idx], after[idx], 0, act[idx], rew[idx], term[idx])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for m in modes:
        window(m, args.warmup)
    res = {m: [] for m in modes}
    for r in range(args.rounds):
        for m in (modes if r % 2 == 0 else modes[::-1]):
            res[m].append(window(m, args.steps))
    kernels = {}
    for m in modes:
        _lib.profile_enable(True)
        window(m, args.steps)
        prof = _lib.profile_collect()
        _lib.profile_enable(False)
        kernels[m] = {name: dict(launches_per_update=e["launches"] / args.steps, us_per_update=1e3 * e["ms"] / args.steps)
                      for name, e in prof.items() if name in KERNELS}
    stats = steppers["dist"].dist_stats.tolist()
    med = {m: _median(v) for m, v in res.items()}
    out = {"batch": B, "dtype": "bf16", "steps_per_window": args.steps, "rounds": args.rounds,
           "ms_per_update": res, "ms_per_update_median": med,
           "window_spread": {m: (max(v) - min(v)) / med[m] for m, v in res.items()},
           "dist_over_dqn": med["dist"] / med["dqn"] - 1, "spread_over_plain": med["spread"] / med["plain"] - 1,
           "loss_launch_us_per_update": kernels, "last_dist_stats": stats,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
