"""Augmentation cost in one process: alternating timed windows of TD updates at batch B (bf16) in a baseline mode and in the mode
--compare names, on the same stepper, both gathering their uint8 frames from the same device pool of `--pool` synthetic tuples.

    --compare shift   "off" (no augmentation, vdqn_pack_input) against "aug": AUG_SHIFT_PAD --pad (8) + AUG_FLIP, i.e. the draw, the
                      action exchange and vdqn_pack_input_aug.  Exit status 1 when the median update is more than --bound (1.5 %) slower.
    --compare color   "shift" (the same shift + mirror) against "color": the three colour keys at --jitter (0.4) on top of it (one more
                      draw launch, vdqn_pack_input_aug_color).
    --compare zoom    "shift" against "zoom": AUG_ZOOM at --zoom (0.25, --aspect: AUG_ZOOM_ASPECT) on top of it (one more draw launch,
                      vdqn_pack_input_aug_zoom: four taps per output pixel where the baseline reads one).
    --compare rotate  "shift" against "rotate": AUG_ROTATE at --rotate (10 degrees) on top of it (one more draw launch; the stepper packs
                      the frames itself with vdqn_pack_input_aug_affine, 2-D tiles, and hands them over as packed_frames).  A third mode,
                      "zoom", runs in the launch-profiler window only: the zoom pack's device time in the same process.
    --compare plain   "off" against "plain", the same unaugmented update: what two modes differ by when nothing differs.

    python tools/bench_aug.py --compare zoom [--batch 256] [--steps 30] [--rounds 6 (shift: 5)] [--out profiles/augzoom_bench.json]
    python tools/bench_aug.py --compare rotate --out profiles/augrot_bench.json

Prints ms/update per mode (every window, the median and the window spread (max - min) / median) and the launch-profiler device time of
the pack and draw launches over the same 2 B frames (a separate window per mode).  The figures to read are the difference between the
medians next to the baseline's own window spread and to the 1.5 % of an update DESIGN 3i allows an augmentation, and the mode's pack
launch next to the baseline's.  The JSON keeps the key names of profiles/aug_bench.json, augcolor_bench.json, augzoom_bench.json and augrot_bench.json."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# --compare -> (baseline mode, compared mode, the baseline's pack launch, the compared mode's)
COMPARISONS = {"plain": ("off", "plain", "pack_input", "pack_input"),
               "shift": ("off", "aug", "pack_input", "pack_input_aug"),
               "color": ("shift", "color", "pack_input_aug", "pack_input_aug_color"),
               "zoom": ("shift", "zoom", "pack_input_aug", "pack_input_aug_zoom"),
               "rotate": ("shift", "rotate", "pack_input_aug", "pack_input_aug_affine")}
KERNELS = ("pack_input", "pack_input_aug", "pack_input_aug_color", "pack_input_aug_zoom", "pack_input_aug_affine", "aug_draw", "aug_draw_color",
           "aug_draw_zoom", "aug_draw_rotate", "aug_swap_actions")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", choices=sorted(COMPARISONS), default="shift")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=None, help="windows per mode: 5 for --compare shift, as profiles/aug_bench.json, else 6")
    ap.add_argument("--pool", type=int, default=512)
    ap.add_argument("--pad", type=int, default=8)
    ap.add_argument("--jitter", type=float, default=0.4)
    ap.add_argument("--zoom", type=float, default=0.25)
    ap.add_argument("--aspect", action="store_true")
    ap.add_argument("--rotate", type=float, default=10.0)
    ap.add_argument("--bound", type=float, default=0.015)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds is None:
        args.rounds = 5 if args.compare == "shift" else 6
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
    base, mode, pack_base_name, pack_mode_name = COMPARISONS[args.compare]
    shift = dict(pad=args.pad, flip=True, flip_actions=[1, 2], seed=1)
    j = args.jitter
    settings = {"off": None, "plain": None, "aug": shift, "shift": shift, "color": dict(shift, brightness=j, contrast=j, saturation=j),
                "zoom": dict(shift, zoom=args.zoom, zoom_aspect=args.aspect), "rotate": dict(shift, rotate=args.rotate)}
    modes = [base, mode]
    profiled = modes + (["zoom"] if args.compare == "rotate" else [])  # (the launch-profiler window alone)
    augs = {m: None if settings[m] is None else Augmenter(B, dev, **settings[m]) for m in profiled}
    uniform_idx = [torch.randint(0, 1 << 30, (B,), device=dev) for _ in range(16)]

    def update(k, m):
        idx = uniform_idx[k % 16] % args.pool
        aug = augs[m]
        if aug is None:
            stp.step(before[idx], after[idx], 0, act[idx], rew[idx], term[idx])
        else:
            params = aug.draw(k)
            stp.step(before[idx], after[idx], 0, aug.actions(act[idx]), rew[idx], term[idx], augment=params, augment_color=aug.color,
                     augment_zoom=aug.zoom if aug.affine is None else None, augment_affine=aug.affine)

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
    for m in profiled:
        for _ in range(args.warmup if m not in modes else 0):
            k += 1
            update(k, m)
        _lib.profile_enable(True)
        for _ in range(args.steps):
            k += 1
            update(k, m)
        torch.cuda.synchronize()
        prof = _lib.profile_collect()
        _lib.profile_enable(False)
        kernels[m] = {name: dict(launches=e["launches"], us_per_update=1e3 * e["ms"] / args.steps) for name, e in prof.items() if name in KERNELS}
    med = {m: sorted(v)[len(v) // 2] for m, v in res.items()}
    spread = {m: (max(v) - min(v)) / med[m] for m, v in res.items()}
    over = med[mode] / med[base] - 1
    pack_base = kernels[base][pack_base_name]["us_per_update"]
    pack_mode = kernels[mode][pack_mode_name]["us_per_update"]
    out = {"batch": B, "dtype": "bf16", "pad": args.pad, "flip": True}
    if args.compare == "color":
        out["jitter"] = j
    if args.compare == "zoom":
        out.update(zoom=args.zoom, zoom_aspect=args.aspect)
    if args.compare == "rotate":
        out.update(rotate=args.rotate, zoom_in_profile_window=args.zoom)
    out.update({"steps_per_window": args.steps, "rounds": args.rounds, "ms_per_update": res, "ms_per_update_median": med, "window_spread": spread,
                f"{mode}_over_{base}": over})
    if args.compare == "shift":  # the one comparison with a threshold: an augmentation against none
        out.update(bound=args.bound, within_bound=over <= args.bound)
    out.update({"frames_per_update": 2 * B, "kernel_us_per_update": kernels, f"{pack_mode_name}_over_{pack_base_name}": pack_mode / pack_base,
                f"{pack_mode_name}_minus_{pack_base_name}_us": pack_mode - pack_base,
                f"{pack_mode_name}_minus_{pack_base_name}_over_update": (pack_mode - pack_base) * 1e-3 / med[base],
                "device": torch.cuda.get_device_name(0)})
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if out.get("within_bound", True) else 1


if __name__ == "__main__":
    sys.exit(main())
