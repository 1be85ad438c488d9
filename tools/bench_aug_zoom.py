"""Random-zoom cost in one process: alternating timed windows of TD updates at batch B (bf16) with the shift / mirror augmentation
alone (AUG_SHIFT_PAD 8, AUG_FLIP on: the baseline) and with AUG_ZOOM at --zoom (0.25) on top of it (one more draw launch,
vdqn_pack_input_aug_zoom instead of vdqn_pack_input_aug: four taps per output pixel where the baseline reads one).  Both modes gather
their uint8 frames from the same device pool of `--pool` synthetic tuples, in the same process, on the same stepper.

    python tools/bench_aug_zoom.py [--batch 256] [--steps 30] [--rounds 6] [--out profiles/augzoom_bench.json]

Prints ms/update per mode (every window, the median and the window spread (max - min) / median) and the launch-profiler device time
of pack_input_aug, pack_input_aug_zoom, aug_draw and aug_draw_zoom over the same 2 B frames (a separate window per mode).  No
threshold: the figures to read are the difference between the medians next to the baseline's own window spread and to the 1.5 % of
an update DESIGN 3i allows an augmentation, and the zoom pack's device time next to pack_input_aug's."""
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
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--pool", type=int, default=512)
    ap.add_argument("--pad", type=int, default=8)
    ap.add_argument("--zoom", type=float, default=0.25)
    ap.add_argument("--aspect", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from video_dqn_amd import _lib, synth
    from video_dqn_amd.augment import Augmenter
    from video_dqn_amd.engine import NetEngine, TDStepper
    dev = "cuda"
    B = args.batch
    net = NetEngine(3, 5, 1, True, "bf16", 2 * B, device=dev)
    net.load_tensors(synth.make_state_dict(7))
    stp = TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True)
    (tup, raw) = synth.make_batch(5, args.pool, 1, structured=True, reward_p=0.05)
    before = torch.from_numpy(raw[0]).to(dev)
    after = torch.from_numpy(raw[1]).to(dev)
    act, rew, term = tup[2].to(dev), tup[3].float().to(dev), tup[4].float().to(dev)
    augs = {"shift": Augmenter(B, dev, pad=args.pad, flip=True, flip_actions=[1, 2], seed=1),
            "zoom": Augmenter(B, dev, pad=args.pad, flip=True, flip_actions=[1, 2], seed=1, zoom=args.zoom, zoom_aspect=args.aspect)}
    uniform_idx = [torch.randint(0, 1 << 30, (B,), device=dev) for _ in range(16)]

    def update(k, mode):
        idx = uniform_idx[k % 16] % args.pool
        aug = augs[mode]
        params = aug.draw(k)
        stp.step(before[idx], after[idx], 0, aug.actions(act[idx]), rew[idx], term[idx], augment=params, augment_zoom=aug.zoom)

    modes = ["shift", "zoom"]
    k = 0
    for m in modes:
        for _ in range(args.warmup):
            k += 1
            update(k, m)
    torch.cuda.synchronize()
    res = {m: [] for m in modes}
    for r in range(args.rounds):
        for m in (modes if r % 2 == 0 else modes[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                k += 1
                update(k, m)
            torch.cuda.synchronize()
            res[m].append((time.perf_counter() - t0) * 1e3 / args.steps)
    kernels = {}
    names = ("pack_input_aug", "pack_input_aug_zoom", "aug_draw", "aug_draw_zoom", "aug_swap_actions")
    for m in modes:
        _lib.profile_enable(True)
        for _ in range(args.steps):
            k += 1
            update(k, m)
        torch.cuda.synchronize()
        prof = _lib.profile_collect()
        _lib.profile_enable(False)
        kernels[m] = {name: dict(launches=e["launches"], us_per_update=1e3 * e["ms"] / args.steps) for name, e in prof.items() if name in names}
    med = {m: sorted(v)[len(v) // 2] for m, v in res.items()}
    spread = {m: (max(v) - min(v)) / med[m] for m, v in res.items()}
    pack_base = kernels["shift"]["pack_input_aug"]["us_per_update"]
    pack_zoom = kernels["zoom"]["pack_input_aug_zoom"]["us_per_update"]
    out = {"batch": B, "dtype": "bf16", "pad": args.pad, "flip": True, "zoom": args.zoom, "zoom_aspect": args.aspect,
           "steps_per_window": args.steps, "rounds": args.rounds,
           "ms_per_update": res, "ms_per_update_median": med, "window_spread": spread, "zoom_over_shift": med["zoom"] / med["shift"] - 1,
           "frames_per_update": 2 * B, "kernel_us_per_update": kernels,
           "pack_input_aug_zoom_over_pack_input_aug": pack_zoom / pack_base, "pack_input_aug_zoom_minus_pack_input_aug_us": pack_zoom - pack_base,
           "pack_input_aug_zoom_minus_pack_input_aug_over_update": (pack_zoom - pack_base) * 1e-3 / med["shift"],
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
