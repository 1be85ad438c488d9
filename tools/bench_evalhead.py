"""Cost of the head algorithms' held-out metrics in one process: per algorithm (IQL, distributional, BCQ) one engine with the
algorithm's head at batch B (bf16) and two TDSteppers on it, one with the algorithm and one without; alternating timed windows of
validation batches through each (`eval_begin` once, then `eval_batch` per batch, `eval_result` at the end of the window: the pass as
the trainer runs it), then the device time of the head metrics launch (launch profiler, a window of its own).  Frames are resident
on the device: the trainer's host-to-device copy of a validation batch is not part of either figure.

    python tools/bench_evalhead.py [--batch 256] [--steps 30] [--rounds 6] [--out profiles/evalhead_bench.json]

Both figures of a pair come from one process and one engine: two processes differ by more than the difference is worth."""
import argparse
import json
import os
import sys
import time

import torch

MODES = {"iql": (dict(value_head=True), dict(iql_expectile=0.7)), "dist": (dict(spread_head=True), dict(distributional=True)),
         "bcq": (dict(policy_head=True), dict(bcq_threshold=0.3))}


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
    (tup, raw) = synth.make_batch(5, args.pool, 1, structured=True, reward_p=0.05)
    before = torch.from_numpy(raw[0]).to(dev)
    after = torch.from_numpy(raw[1]).to(dev)
    act, rew, term = tup[2].to(dev), tup[3].float().to(dev), tup[4].float().to(dev)
    idxs = [torch.randint(0, args.pool, (B,), device=dev) for _ in range(16)]
    out = {"batch": B, "dtype": "bf16", "steps_per_window": args.steps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    for algo, (net_kw, step_kw) in MODES.items():
        net = NetEngine(3, 5, 1, True, "bf16", 2 * B, device=dev, **net_kw)
        net.load_tensors(synth.make_state_dict(7))
        steppers = {"plain": TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True),
                    "head": TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, **step_kw)}
        k = [0]
        last = {}

        def window(mode, steps):
            stp = steppers[mode]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stp.eval_begin()
            for _ in range(steps):
                k[0] += 1
                idx = idxs[k[0] % 16]
                stp.eval_batch(before[idx], after[idx], 0, act[idx], rew[idx], term[idx])
            last[mode] = stp.eval_result()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / steps

        modes = ["plain", "head"]
        for m in modes:
            window(m, args.warmup)
        res = {m: [] for m in modes}
        for r in range(args.rounds):
            for m in (modes if r % 2 == 0 else modes[::-1]):
                res[m].append(window(m, args.steps))
        _lib.profile_enable(True)
        window("head", args.steps)
        prof = _lib.profile_collect()
        _lib.profile_enable(False)
        launch = {name: dict(launches_per_batch=e["launches"] / args.steps, us_per_batch=1e3 * e["ms"] / args.steps)
                  for name, e in prof.items() if name in ("td_eval", f"td_eval_{algo}")}
        med = {m: _median(v) for m, v in res.items()}
        head = last["head"]["head"]
        out[algo] = {"ms_per_eval_batch": res, "ms_median": med, "window_spread": {m: (max(v) - min(v)) / med[m] for m, v in res.items()},
                     "head_over_plain": med["head"] / med["plain"], "added_us_per_batch": 1e3 * (med["head"] - med["plain"]),
                     "metrics_launches": launch,
                     "last_pass_head": {key: head[key] for key in steppers["head"].algo.eval_slots + steppers["head"].algo.eval_sample_slots}}
        del steppers, net
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
