"""Cost of the frame gradient in one process.

1. The operator at n images in bf16: device time (HIP events around runs of launches) of the fused launch, vdqn_stem_input_grad,
   against the unfused composition — vdqn_maxpool_bwd into an f32 tensor plus the f32 kernel (vdqn_conv2d's data-gradient mode does
   not take the 64 -> 16-channel packed geometry) — and against the byte floor (g_pool + idx + output) at 5 TB/s, the HBM rate the
   other tools of this directory use.  Windows of the two alternate; medians and the spread of the windows are reported.
2. The module at batch B: `model.input_gradient` against `backward_from_dq` alone (the same forward workspace, so the difference is
   the one extra launch and its output allocation), alternating windows again.
3. The cosine between the bf16 and the f32 engine's input gradient on one batch of 8 (DESIGN section 3 quotes it).

    python tools/bench_input_grad.py [--n 256] [--batch 64] [--reps 10] [--rounds 6] [--out profiles/input_grad_bench.json]

The baseline is never a separate run: two processes differ by more than the effect looked for."""
import argparse
import json
import os
import sys

import torch


def _median(v):
    return sorted(v)[len(v) // 2]


def _timed(fn, reps):
    """ms per call: device time between two events around `reps` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _alternate(fns, reps, rounds, warmup=2):
    names = list(fns)
    for n in names:
        for _ in range(warmup):
            fns[n]()
    torch.cuda.synchronize()
    res = {n: [] for n in names}
    for r in range(rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            res[n].append(_timed(fns[n], reps))
    med = {n: _median(v) for n, v in res.items()}
    return dict(ms=res, ms_median=med, window_spread={n: (max(v) - min(v)) / med[n] for n, v in res.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from video_dqn_amd import ops, synth
    from video_dqn_amd.model import HabitatDQNMultiAction
    dev = "cuda"
    n = args.n
    g = torch.Generator().manual_seed(1)
    g_pool = (torch.randn((n, 56, 56, 64), generator=g) * (torch.rand((n, 56, 56, 64), generator=g) < 0.5)).to(torch.bfloat16).to(dev)
    kh = torch.randint(1, 3, (n, 56, 56, 64), generator=g)
    kw = torch.randint(1, 3, (n, 56, 56, 64), generator=g)
    idx = (kh * 3 + kw).to(torch.uint8).to(dev)  # codes whose target lies inside the image at every position
    wt = ((torch.rand((64, 4, 1, 64), generator=g) * 2 - 1) * 0.2).to(torch.bfloat16).to(dev)
    g32, w32 = g_pool.float(), wt.float()
    op = _alternate({"fused_bf16": lambda: ops.stem_input_grad(g_pool, idx, wt),
                     "unfused_f32": lambda: ops.stem_input_grad(g32, idx, w32)}, args.reps, args.rounds)
    floor_bytes = n * (56 * 56 * 64 * 3 + 3 * 224 * 224 * 4)
    op.update(n_img=n, byte_floor_bytes=floor_bytes, byte_floor_ms_at_5TBs=floor_bytes / 5e12 * 1e3,
              fused_over_floor=op["ms_median"]["fused_bf16"] / (floor_bytes / 5e12 * 1e3),
              unfused_over_fused=op["ms_median"]["unfused_f32"] / op["ms_median"]["fused_bf16"])
    del g32, w32, g_pool, idx
    torch.cuda.empty_cache()

    B = args.batch
    model = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype="bf16", device=dev, max_batch=B)
    model.load_state_dict(synth.make_state_dict(7))
    model.eval()
    frames = torch.from_numpy(synth.make_frames_uint8(5, "f", B, 1, structured=True)).to(dev)
    dq = torch.from_numpy(synth.uniform(6, "dq", (B, 15), -1.0, 1.0)).to(dev)
    eng = model.engine
    packed = model._packed_with_dgrad()
    _, acts = eng.forward_saved(frames, 0, B, packed)
    mod = _alternate({"backward_from_dq": lambda: eng.backward_from_dq(acts, packed, dq, B),
                      "backward_from_dq_with_gx": lambda: eng.backward_from_dq(acts, packed, dq, B, want_input_grad=True),
                      "input_gradient": lambda: model.input_gradient(frames, dq)}, args.reps, args.rounds)
    m = mod["ms_median"]
    mod.update(batch=B, input_grad_launch_share_of_backward=(m["backward_from_dq_with_gx"] - m["backward_from_dq"]) / m["backward_from_dq_with_gx"],
               input_gradient_over_backward=m["input_gradient"] / m["backward_from_dq"])

    f32 = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype="f32", device=dev, max_batch=8)
    f32.load_state_dict(synth.make_state_dict(7))
    a = model.input_gradient(frames[:8], dq[:8]).double().flatten()
    b = f32.input_gradient(frames[:8], dq[:8]).double().flatten()
    cosine = float((a @ b) / (a.norm() * b.norm()))

    out = {"dtype": "bf16", "reps_per_window": args.reps, "rounds": args.rounds, "operator": op, "module": mod,
           "cosine_bf16_vs_f32_batch8": cosine, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
