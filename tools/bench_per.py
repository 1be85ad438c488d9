"""Prioritized replay cost in one process: alternating timed windows of TD updates with and without PER at batch B (bf16), with the
priority table at N = 100 000 and 1 000 000 samples.  Frames come from a device pool of `--pool` synthetic tuples, gathered by
idx mod pool (what DeviceFrameStore.gather does on a resident dataset), so both modes pay the same gather.

    python tools/bench_per.py [--batch 256] [--steps 30] [--rounds 3] [--out profiles/per_bench.json]

Prints ms/update per mode and N, and the device time of the new launches (launch profiler, a separate window)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pool", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from video_dqn_amd import _lib, synth
    from video_dqn_amd.engine import NetEngine, TDStepper
    from video_dqn_amd.replay import PrioritizedSampler
    dev = "cuda"
    B = args.batch
    net = NetEngine(3, 5, 1, True, "bf16", 2 * B, device=dev)
    net.load_tensors(synth.make_state_dict(7))
    stp = TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True)
    (tup, raw) = synth.make_batch(5, args.pool, 1, structured=True, reward_p=0.05)
    before = torch.from_numpy(raw[0]).to(dev)
    after = torch.from_numpy(raw[1]).to(dev)
    act, rew, term = tup[2].to(dev), tup[3].float().to(dev), tup[4].float().to(dev)
    samplers = {n: PrioritizedSampler(n, B, dev, alpha=0.6, beta=0.4, num_steps=100000, seed=1) for n in (100000, 1000000)}
    uniform_idx = [torch.randint(0, 1 << 30, (B,), device=dev) for _ in range(16)]

    def update(k, smp):
        if smp is None:
            idx = uniform_idx[k % 16] % args.pool
            stp.step(before[idx], after[idx], 0, act[idx], rew[idx], term[idx])
        else:
            idx, w = smp.sample(k)
            j = idx % args.pool
            stp.step(before[j], after[j], 0, act[j], rew[j], term[j], weights=w, td_error=smp.err)
            smp.update()

    modes = [("off", None)] + [(f"per_n{n}", s) for n, s in samplers.items()]
    k = 0
    for _, smp in modes:
        for _ in range(args.warmup):
            k += 1
            update(k, smp)
    torch.cuda.synchronize()
    res = {m: [] for m, _ in modes}
    for r in range(args.rounds):
        for m, smp in (modes if r % 2 == 0 else modes[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                k += 1
                update(k, smp)
            torch.cuda.synchronize()
            res[m].append((time.perf_counter() - t0) * 1e3 / args.steps)
    kernels = {}
    for m, smp in modes[1:]:
        _lib.profile_enable(True)
        for _ in range(args.steps):
            k += 1
            update(k, smp)
        torch.cuda.synchronize()
        prof = _lib.profile_collect()
        _lib.profile_enable(False)
        kernels[m] = {name: dict(launches=e["launches"], us_per_update=1e3 * e["ms"] / args.steps)
                      for name, e in prof.items() if name in ("per_blocksum", "per_sample", "per_update", "td_loss_w", "td_loss")}
    out = {"batch": B, "dtype": "bf16", "steps_per_window": args.steps, "rounds": args.rounds,
           "ms_per_update": {m: v for m, v in res.items()},
           "ms_per_update_median": {m: sorted(v)[len(v) // 2] for m, v in res.items()},
           "per_over_off": {m: sorted(v)[len(v) // 2] / sorted(res["off"])[len(res["off"]) // 2] - 1 for m, v in res.items() if m != "off"},
           "kernel_us_per_update": kernels, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
