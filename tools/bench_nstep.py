"""Cost of n-step returns in one process: alternating timed windows of TD updates at batch B (bf16) of an N_STEP 1 loop — the
resident store's gather and the update as they are without the feature, the baseline — against an N_STEP 3 loop (one chain walk,
`after` gathered from each chain's last row, the per-sample discount in the loss launch) on the same engine and the same
synthetic resident store, as tools/bench_cql.py alternates its variants; then the device time of the walk and of the loss launch of
each loop (launch profiler, windows of their own).

    python tools/bench_nstep.py [--batch 256] [--steps 30] [--rounds 6] [--n 3] [--out profiles/nstep_bench.json]

The baseline is never a separate run: two processes differ by more than the effect looked for."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

KERNELS = ("nstep_walk", "td_loss", "td_loss_w", "td_loss_cql")


def _median(v):
    return sorted(v)[len(v) // 2]


def synthetic_store(pool, episode, dev, seed=5):
    """A DeviceFrameStore over `pool` random frames without a shard directory: one row per frame i of an episode of `episode` frames,
    (before = i, after = i + 3) as dataset/process_episodes_real.py writes them, sparse rewards with terminal = reward."""
    from video_dqn_amd.nstep import successors
    from video_dqn_amd.shards import DeviceFrameStore
    rng = np.random.default_rng(seed)
    before, after = [], []
    for e0 in range(0, pool, episode):
        e1 = min(pool, e0 + episode)
        for i in range(e0, e1 - 3):
            before.append(i)
            after.append(i + 3)
    before, after = np.asarray(before, np.int64), np.asarray(after, np.int64)
    n = len(before)
    store = object.__new__(DeviceFrameStore)
    store.device, store.nf = torch.device(dev), 1
    store.frames = torch.randint(0, 256, (pool, 224, 224, 3), dtype=torch.uint8, device=dev)
    store.before, store.after = torch.from_numpy(before).view(n, 1).to(dev), torch.from_numpy(after).view(n, 1).to(dev)
    rew = torch.from_numpy((rng.random((n, 5)) < 0.05).astype(np.float32))
    store.act = torch.from_numpy(rng.integers(0, 3, n)).to(dev)
    store.rew, store.term = rew.to(dev), rew.clone().to(dev)
    store.valid, store.gt = torch.ones(n, 5, device=dev), torch.full((n, 5), float("nan"), device=dev)
    return store, successors(before, after)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--pool", type=int, default=2048)
    ap.add_argument("--episode", type=int, default=256)
    ap.add_argument("--n", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from video_dqn_amd import _lib, synth
    from video_dqn_amd.engine import NetEngine, TDStepper
    from video_dqn_amd.nstep import NStepWalker, chain_shares
    dev = "cuda"
    B = args.batch
    net = NetEngine(3, 5, 1, True, "bf16", 2 * B, device=dev)
    net.load_tensors(synth.make_state_dict(7))
    store, next_row = synthetic_store(args.pool, args.episode, dev)
    walker = NStepWalker(next_row, store.rew, store.term, B, args.n, 0.99, dev)
    modes = ["n1", f"n{args.n}"]
    steppers = {m: TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True) for m in modes}
    idxs = [torch.randint(0, len(store), (B,), device=dev) for _ in range(16)]
    k = [0]

    def window(mode, steps):
        stp = steppers[mode]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            k[0] += 1
            idx = idxs[k[0] % 16]
            batch = store.gather(idx, walker=(None if mode == "n1" else walker))
            stp.step(batch.before, batch.after, 0, batch.act, batch.rew, batch.term, discount=batch.discount)
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
    med = {m: _median(v) for m, v in res.items()}
    out = {"batch": B, "dtype": "bf16", "n_step": args.n, "steps_per_window": args.steps, "rounds": args.rounds,
           "rows": len(store), "frames": args.pool, "chain_shares": chain_shares(next_row, args.n),
           "mean_rows_walked": float(walker.steps.float().mean().item()),
           "ms_per_update": res, "ms_per_update_median": med,
           "window_spread": {m: (max(v) - min(v)) / med[m] for m, v in res.items()},
           "nstep_over_one_step": med[modes[1]] / med["n1"] - 1,
           "launch_us_per_update": kernels, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
