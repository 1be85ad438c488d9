"""Cost of soft (Polyak) target updates in one process: alternating timed windows of TD updates at batch B (bf16) through a
TDStepper with target_tau = 0 — the update as it is without the feature, the baseline — and one with target_tau = 0.005 on the
same engine (as tools/bench_cql.py alternates its variants), then the device time of the launches that differ (launch profiler,
windows of their own): `adam` against `adam_polyak`, and `fold_weights`, which the soft update launches once more per update.

    python tools/bench_polyak.py [--batch 256] [--steps 30] [--rounds 6] [--out profiles/polyak_bench.json]

The baseline is never a separate run: two processes differ by more than the effect looked for."""
import argparse
import json
import os
import sys
import time

import torch

KERNELS = ("adam", "adam_scaled", "adam_polyak", "polyak", "fold_weights")


def _median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--pool", type=int, default=512)
    ap.add_argument("--tau", type=float, default=0.005)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from video_dqn_amd import _lib, synth
    from video_dqn_amd.engine import NetEngine, TDStepper
    dev = "cuda"
    B = args.batch
    net = NetEngine(3, 5, 1, True, "bf16", 2 * B, device=dev)
    net.load_tensors(synth.make_state_dict(7))
    steppers = {"tau0": TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, target_tau=0.0),
                "tau": TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, target_tau=args.tau)}
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
    kernels, tables = {}, {}
    for m in modes:
        _lib.profile_enable(True)
        window(m, args.steps)
        prof = _lib.profile_collect()
        _lib.profile_enable(False)
        per_update = {name: dict(launches_per_update=e["launches"] / args.steps, us_per_update=1e3 * e["ms"] / args.steps)
                      for name, e in prof.items()}
        kernels[m] = {name: e for name, e in per_update.items() if name in KERNELS}
        tables[m] = per_update

    def us(mode, names):
        return sum(kernels[mode].get(n, {}).get("us_per_update", 0.0) for n in names)
    # every launch whose device time moved by more than 5 us per update between the two profiled windows (the whole table, so that
    # a difference the two expected launches do not explain can be named)
    moved = {name: tables["tau"].get(name, {}).get("us_per_update", 0.0) - tables["tau0"].get(name, {}).get("us_per_update", 0.0)
             for name in sorted(set(tables["tau"]) | set(tables["tau0"]))}
    moved = {name: d for name, d in moved.items() if abs(d) > 5.0}

    med = {m: _median(v) for m, v in res.items()}
    out = {"batch": B, "dtype": "bf16", "tau": args.tau, "steps_per_window": args.steps, "rounds": args.rounds,
           "ms_per_update": res, "ms_per_update_median": med,
           "window_spread": {m: (max(v) - min(v)) / med[m] for m, v in res.items()},
           "tau_minus_tau0_ms_per_update": med["tau"] - med["tau0"],
           "tau_over_tau0": med["tau"] / med["tau0"] - 1,
           "launch_us_per_update": kernels,
           "adam_launches_delta_us_per_update": us("tau", ("adam", "adam_scaled", "adam_polyak")) - us("tau0", ("adam", "adam_scaled", "adam_polyak")),
           "fold_weights_delta_us_per_update": us("tau", ("fold_weights",)) - us("tau0", ("fold_weights",)),
           "launches_that_moved_more_than_5us": moved,
           "params_numel": int(net.params_numel), "trainable_numel": int(net.trainable_numel),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
