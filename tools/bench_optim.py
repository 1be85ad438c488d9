"""Cost of gradient clipping, weight decay and the learning-rate schedule in one process: alternating timed windows of TD updates
at batch B (bf16) with the keys off, clipping only, decay + schedule only, and all three (as tools/ab_inproc.py alternates its
variants), then the device time of the new launches next to `adam`'s (launch profiler, windows of their own).

    python tools/bench_optim.py [--batch 256] [--steps 30] [--rounds 4] [--out profiles/optim_bench.json]
                                [--parent-json FILE ...]

The parent commit's plain update is measured by the same file on a checkout of that commit (it only uses what that commit has):

    python tools/bench_optim.py --root <parent checkout> --plain-only --out parent_plain.json

once before and once after the main run; `--parent-json` (with `--merge <result>` afterwards) merges those into the result (ratios against their median, and the
parent's own window spread, which is what a difference has to exceed to mean anything)."""
import argparse
import json
import os
import sys
import time

import torch

KEYS_OFF = dict(grad_clip_norm=0.0, weight_decay=0.0, schedule=False)
MODES = [("off", KEYS_OFF),
         ("clip", dict(grad_clip_norm=1.0, weight_decay=0.0, schedule=False)),
         ("decay_schedule", dict(grad_clip_norm=0.0, weight_decay=0.01, schedule=True)),
         ("all", dict(grad_clip_norm=1.0, weight_decay=0.01, schedule=True))]
KERNELS = ("adam", "adam_scaled", "grad_sumsq", "clip_finalize")


def _median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--pool", type=int, default=512)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package is measured")
    ap.add_argument("--plain-only", action="store_true", help="time the plain update alone (works on the parent commit too)")
    ap.add_argument("--parent-json", action="append", default=[], help="result of a --plain-only run on the parent commit")
    ap.add_argument("--merge", default=None, help="a result of this tool: only (re)do the --parent-json merge on it, nothing is measured")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.merge:
        with open(args.merge) as f:
            out = json.load(f)
        return finish(out, args)
    sys.path.insert(0, os.path.abspath(args.root))
    from video_dqn_amd import _lib, synth
    from video_dqn_amd.engine import NetEngine, TDStepper
    dev = "cuda"
    B = args.batch
    net = NetEngine(3, 5, 1, True, "bf16", 2 * B, device=dev)
    net.load_tensors(synth.make_state_dict(7))
    kw = {} if args.plain_only else dict(grad_clip_norm=1.0)  # (allocates the norm workspace; the modes below switch the keys)
    stp = TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, **kw)
    (tup, raw) = synth.make_batch(5, args.pool, 1, structured=True, reward_p=0.05)
    before = torch.from_numpy(raw[0]).to(dev)
    after = torch.from_numpy(raw[1]).to(dev)
    act, rew, term = tup[2].to(dev), tup[3].float().to(dev), tup[4].float().to(dev)
    idxs = [torch.randint(0, args.pool, (B,), device=dev) for _ in range(16)]
    modes = MODES[:1] if args.plain_only else MODES
    if not args.plain_only:
        from video_dqn_amd.optim import lr_at

        def lr_fn(t):
            return lr_at(t, 1e-4, 1000, "cosine", 0.1, 100000)

    def set_mode(keys):
        if args.plain_only:
            return
        stp.grad_clip_norm, stp.weight_decay = keys["grad_clip_norm"], keys["weight_decay"]
        stp.lr_fn = lr_fn if keys["schedule"] else None
        stp.lr = 1e-4

    k = [0]

    def window(keys, steps):
        set_mode(keys)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            k[0] += 1
            idx = idxs[k[0] % 16]
            stp.step(before[idx], after[idx], 0, act[idx], rew[idx], term[idx])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for _, keys in modes:
        window(keys, args.warmup)
    res = {m: [] for m, _ in modes}
    for r in range(args.rounds):
        for m, keys in (modes if r % 2 == 0 else modes[::-1]):
            res[m].append(window(keys, args.steps))
    kernels = {}
    for m, keys in modes:
        _lib.profile_enable(True)
        window(keys, args.steps)
        prof = _lib.profile_collect()
        _lib.profile_enable(False)
        kernels[m] = {name: dict(launches_per_update=e["launches"] / args.steps, us_per_update=1e3 * e["ms"] / args.steps,
                                 gbytes_per_s=(e["bytes"] / (e["ms"] * 1e6) if e["ms"] > 0 else None))
                      for name, e in prof.items() if name in KERNELS}
    med = {m: _median(v) for m, v in res.items()}
    out = {"batch": B, "dtype": "bf16", "steps_per_window": args.steps, "rounds": args.rounds, "trainable_numel": net.trainable_numel,
           "ms_per_update": res, "ms_per_update_median": med,
           "window_spread": {m: (max(v) - min(v)) / med[m] for m, v in res.items()},
           "over_off": {m: med[m] / med["off"] - 1 for m in med if m != "off"},
           "kernel_us_per_update": kernels, "device": torch.cuda.get_device_name(0)}
    finish(out, args)


def finish(out, args):
    med = out["ms_per_update_median"]
    if args.parent_json:
        windows = []
        for path in args.parent_json:
            with open(path) as f:
                windows += json.load(f)["ms_per_update"]["off"]
        pm = _median(windows)
        out["parent_plain"] = {"ms_per_update": windows, "ms_per_update_median": pm, "window_spread": (max(windows) - min(windows)) / pm}
        out["over_parent_plain"] = {m: med[m] / pm - 1 for m in med}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
