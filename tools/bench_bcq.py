"""Cost of discrete BCQ in one process: alternating timed windows of TD updates at batch B (bf16) through a TDStepper with
bcq_threshold = -1 — the Double-DQN update, the parent's launches — and one with bcq_threshold = 0.3 on the same policy-head engine
(as tools/bench_iql.py alternates its variants), then the device time of the loss launch of each (launch profiler, windows of
their own).  The three forward passes and the backward are the same either way, so the expected difference is the loss launch alone.

    python tools/bench_bcq.py [--batch 256] [--steps 30] [--rounds 6] [--out profiles/bcq_bench.json]

The baseline is never a separate run: two processes differ by more than the effect looked for."""
import argparse
import json
import os
import sys
import time

import torch

KERNELS = ("td_loss", "td_loss_bcq")


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
    net = NetEngine(3, 5, 1, True, "bf16", 2 * B, device=dev, policy_head=True)
    net.load_tensors(synth.make_state_dict(7))
    g = torch.Generator().manual_seed(3)
    net.view("policy.weight").copy_((torch.rand(3, 256, generator=g) * 2 - 1) / 16)
    net.view("policy.bias").copy_((torch.rand(3, generator=g) * 2 - 1) / 16)
    net.mark_dirty()
    steppers = {"dqn": TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, bcq_threshold=-1.0),
                "bcq": TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, bcq_threshold=0.3)}
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
    stats = steppers["bcq"].bcq_stats.tolist()
    med = {m: _median(v) for m, v in res.items()}
    out = {"batch": B, "dtype": "bf16", "steps_per_window": args.steps, "rounds": args.rounds,
           "ms_per_update": res, "ms_per_update_median": med,
           "window_spread": {m: (max(v) - min(v)) / med[m] for m, v in res.items()},
           "bcq_over_dqn": med["bcq"] / med["dqn"] - 1,
           "loss_launch_us_per_update": kernels, "last_bcq_stats": stats,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
