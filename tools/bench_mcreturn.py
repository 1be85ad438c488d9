"""Cost of the Monte-Carlo return floor and the calibrated penalty in one process: alternating timed windows of TD updates at batch
B (bf16) of a loop with both keys off — the resident store's gather and the CQL update as they are without the feature, the
baseline — against a loop with both on (G gathered at the sampled rows, the loss launch vdqn_td_loss_mc with both flags) on the same
engine and the same synthetic resident store, as tools/bench_nstep.py alternates its variants; then the device time of the loss
launch either way (launch profiler, windows of their own) and of the one-off table build at N rows.

    python tools/bench_mcreturn.py [--batch 256] [--steps 30] [--rounds 6] [--table-rows 1000000] [--table-rounds 12]
                                   [--out profiles/mcreturn_bench.json]

The baseline is never a separate run: two processes differ by more than the effect looked for."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

KERNELS = ("td_loss_cql", "td_loss_cql_mc", "mc_returns")


def _median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--pool", type=int, default=2048)
    ap.add_argument("--episode", type=int, default=256)
    ap.add_argument("--table-rows", type=int, default=1000000)
    ap.add_argument("--table-cat", type=int, default=5)
    ap.add_argument("--table-rounds", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tools"))
    from bench_nstep import synthetic_store
    from video_dqn_amd import _lib, ops, synth
    from video_dqn_amd.engine import NetEngine, TDStepper
    from video_dqn_amd.mcreturn import ReturnTable
    dev = "cuda"
    B = args.batch
    net = NetEngine(3, 5, 1, True, "bf16", 2 * B, device=dev)
    net.load_tensors(synth.make_state_dict(7))
    store, next_row = synthetic_store(args.pool, args.episode, dev)
    table = ReturnTable(next_row, store.rew, store.term, 0.99, dev)
    modes = ["off", "on"]
    steppers = {"off": TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, cql_alpha=1.0),
                "on": TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, cql_alpha=1.0, mc_floor=True, cql_calibrated=True)}
    idxs = [torch.randint(0, len(store), (B,), device=dev) for _ in range(16)]
    k = [0]

    def window(mode, steps):
        stp = steppers[mode]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            k[0] += 1
            idx = idxs[k[0] % 16]
            batch = store.gather(idx, returns=(table if mode == "on" else None))
            stp.step(batch.before, batch.after, 0, batch.act, batch.rew, batch.term, mc_return=batch.mc_return)
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
    mc_stats = [float(v) for v in steppers["on"].mc_stats.tolist()]

    # the one-off table build: chains i -> i + 3 in episodes of `episode` rows, sparse binary rewards with terminal = reward
    N, C, R = args.table_rows, args.table_cat, args.table_rounds
    rng = np.random.default_rng(5)
    nxt = np.arange(N, dtype=np.int64) + 3
    nxt[(nxt >= N) | (nxt // args.episode != np.arange(N) // args.episode)] = -1
    rew = torch.from_numpy((rng.random((N, C)) < 0.05).astype(np.float32)).to(dev)
    term, nxt_d = rew.clone(), torch.from_numpy(nxt.astype(np.int32)).to(dev)
    ws = torch.empty(int(_lib.load().vdqn_mc_returns_workspace_bytes(N, C)), dtype=torch.uint8, device=dev)
    G = torch.empty((N, C), dtype=torch.float32, device=dev)
    builds = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.mc_returns(nxt_d, rew, term, gamma=0.99, rounds=R, out=G, workspace=ws)
        torch.cuda.synchronize()
        builds.append((time.perf_counter() - t0) * 1e3)
    nc = N * C
    moved = nc * 4 * (4 + 6 * R) + N * 4 * (2 + 3 * R)  # bytes read and written, the gathers counted once

    med = {m: _median(v) for m, v in res.items()}
    out = {"batch": B, "dtype": "bf16", "cql_alpha": 1.0, "steps_per_window": args.steps, "rounds": args.rounds,
           "rows": len(store), "frames": args.pool, "table_rounds": table.rounds,
           "ms_per_update": res, "ms_per_update_median": med,
           "window_spread": {m: (max(v) - min(v)) / med[m] for m, v in res.items()},
           "on_over_off": med["on"] / med["off"] - 1,
           "launch_us_per_update": kernels, "mc_stats_last_update": mc_stats,
           "table_build": {"rows": N, "n_cat": C, "rounds": R, "ms": builds, "ms_median": _median(builds),
                           "workspace_bytes": ws.numel(), "gb_per_s_at_median": moved / (_median(builds) * 1e-3) / 1e9,
                           "table_max": float(G.max().item())},
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
