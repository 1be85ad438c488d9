#!/usr/bin/env python
"""Speed of the three compute modes INSIDE one process: TD updates (extra_capacity, F = 1) on an f32, a bf16x3 and a bf16 engine,
alternating window by window as tools/ab_inproc.py does (the box's slow drift hits every mode alike); medians over the rounds, then
one profiled window per mode (vdqn_profile_collect) for the per-kernel table.  Writes a JSON record.
    python tools/bench_precision.py [--rounds 8] [--batches 64,256] [--out profiles/bf16x3_bench_precision.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = ("f32", "bf16x3", "bf16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--updates", type=float, default=0.25, help="seconds of f32 updates per window (the other modes run as many updates)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from video_dqn_amd import _lib, engine as eng, synth
    dev = torch.device("cuda", 0)
    record = {"tool": "tools/bench_precision.py", "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "batches": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        g = torch.Generator(device=dev)
        g.manual_seed(1234)
        pool = []
        for _ in range(4):
            b_ = torch.randint(0, 256, (B, 1, 224, 224, 3), dtype=torch.uint8, device=dev, generator=g)
            a_ = torch.randint(0, 256, (B, 1, 224, 224, 3), dtype=torch.uint8, device=dev, generator=g)
            act_ = torch.randint(0, 3, (B,), dtype=torch.int64, device=dev, generator=g)
            rew_ = (torch.rand((B, 5), device=dev, generator=g) < 0.05).float()
            pool.append((b_, a_, act_, rew_, rew_.clone()))
        steppers = {}
        for m in MODES:
            net = eng.NetEngine(3, 5, 1, True, m, 2 * B, device=dev)
            net.load_tensors(synth.make_state_dict(4, extra_capacity=True, num_frames=1))
            steppers[m] = eng.TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, target_update_interval=1000000)
        k = {"i": 0}

        def step(m):
            b_, a_, act_, rew_, term_ = pool[k["i"] % 4]
            k["i"] += 1
            steppers[m].step(b_, a_, 0, act_, rew_, term_)

        def window(m, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                step(m)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3

        for m in MODES:  # ramp
            window(m, 10)
        n_win = max(4, int(args.updates * 1e3 / window("f32", 4)))
        res = {m: [] for m in MODES}
        for r in range(args.rounds):
            for m in (MODES if r % 2 == 0 else MODES[::-1]):
                window(m, 2)
                dt = window(m, n_win)
                res[m].append(dt)
                print(f"B={B} round {r} {m:7s} {dt:8.3f} ms  {B / dt * 1e3:9.1f} tuples/s", flush=True)
        kernels = {}
        for m in MODES:
            window(m, 2)
            _lib.profile_collect()
            _lib.profile_enable(True)
            window(m, 4)
            rows = _lib.profile_collect()
            _lib.profile_enable(False)
            kernels[m] = {name: {"ms_per_update": round(v["ms"] / 4, 4), "launches_per_update": v["launches"] / 4,
                                 "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) if v["ms"] > 0 else None}
                          for name, v in sorted(rows.items(), key=lambda kv: -kv[1]["ms"])}
        med = {m: statistics.median(res[m]) for m in MODES}
        entry = {"updates_per_window": n_win,
                 "ms_per_update": {m: {"median": round(med[m], 4), "min": round(min(res[m]), 4), "max": round(max(res[m]), 4),
                                       "windows": [round(x, 4) for x in res[m]]} for m in MODES},
                 "tuples_per_s": {m: round(B / med[m] * 1e3, 1) for m in MODES},
                 "bf16x3_over_f32": round(med["bf16x3"] / med["f32"], 4),
                 "bf16x3_over_bf16": round(med["bf16x3"] / med["bf16"], 4),
                 "kernels": kernels}
        record["batches"][str(B)] = entry
        print(f"---- B={B} medians: " + ", ".join(f"{m} {med[m]:.3f} ms" for m in MODES) +
              f"; bf16x3 / f32 = {entry['bf16x3_over_f32']:.3f}", flush=True)
        for m in MODES:
            top = list(kernels[m].items())[:8]
            print(f"  {m:7s} " + "; ".join(f"{n} {v['ms_per_update']:.3f}" for n, v in top))
        del steppers
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
