"""Cost of attribution in one process (bf16 engine).

1. The data-gradient-only backward at batch B (64 and 256): `NetEngine.backward_data` against `backward_from_dq(want_input_grad=True)`,
   the full training backward plus the stem's data-gradient launch, on the same saved activations.  Device time (HIP events around
   runs of calls); windows of the two alternate; medians and the spread of the windows are reported.
2. Integrated gradients with 32 steps at B = 8: `model.integrated_gradients` (perturbed operand built by the pack, 64-sample forward /
   backward pairs, sum on the device) against the host loop it replaces — per step the path point built with torch, one forward and
   one FULL backward with the frame gradient (what `input_gradient` cost before the data-only backward), the sum and the final
   product in torch.

    python tools/bench_attribution.py [--batches 64,256] [--ig-batch 8] [--steps 32] [--max-batch 64] [--reps 5] [--rounds 6]
                                      [--out profiles/attribution_bench.json]

The baseline is never a separate run: two processes differ by more than the effect looked for."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_input_grad import _alternate  # noqa: E402  (the alternating-window timer)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--ig-batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from video_dqn_amd import ops, synth
    from video_dqn_amd.model import HabitatDQNMultiAction
    dev = "cuda"

    def module(max_batch):
        m = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype="bf16", device=dev, max_batch=max_batch)
        m.load_state_dict(synth.make_state_dict(7))
        m.eval()
        return m

    backward = {}
    for B in [int(b) for b in args.batches.split(",")]:
        model = module(B)
        eng = model.engine
        frames = torch.from_numpy(synth.make_frames_uint8(5, "f", B, 1, structured=True)).to(dev)
        dq = torch.from_numpy(synth.uniform(6, "dq", (B, 15), -1.0, 1.0)).to(dev)
        packed = model._packed_with_dgrad()
        _, acts = eng.forward_saved(frames, 0, B, packed)
        r = _alternate({"backward_from_dq_with_gx": lambda: eng.backward_from_dq(acts, packed, dq, B, want_input_grad=True),
                        "backward_data": lambda: eng.backward_data(acts, packed, dq, B)}, args.reps, args.rounds)
        full, gx = eng.backward_from_dq(acts, packed, dq, B, want_input_grad=True)
        r.update(batch=B, same_bits=bool(torch.equal(gx.view(torch.int32), eng.backward_data(acts, packed, dq, B).view(torch.int32))),
                 full_over_data=r["ms_median"]["backward_from_dq_with_gx"] / r["ms_median"]["backward_data"])
        backward[str(B)] = r
        del model, eng, acts, packed, full, gx
        torch.cuda.empty_cache()

    B, steps = args.ig_batch, args.steps
    model = module(args.max_batch)
    eng = model.engine
    u8 = torch.from_numpy(synth.make_frames_uint8(8, "f", B, 1, structured=True)).to(dev)
    x = ops.norm_pixel([0, 0, 0])
    black = torch.tensor(x, device=dev).view(1, 1, 3, 1, 1)
    with torch.no_grad():
        xn = ((u8.float() / 255.0).permute(0, 1, 4, 2, 3) - torch.tensor([0.485, 0.456, 0.406], device=dev).view(1, 1, 3, 1, 1)) \
            / torch.tensor([0.229, 0.224, 0.225], device=dev).view(1, 1, 3, 1, 1)
        xn = xn.contiguous()
        q = model(xn)
    dq = torch.zeros_like(q)
    dq[torch.arange(B, device=dev), 3, q[:, 3].argmax(-1)] = 1.0
    dq = dq.view(B, -1)

    def host_loop():
        packed = model._packed_with_dgrad()
        acc = torch.zeros_like(xn)
        for k in range(steps):
            xk = (black + ((k + 0.5) / steps) * (xn - black)).contiguous()
            _, acts = eng.forward_saved(xk, 1, B, packed)
            _, gx = eng.backward_from_dq(acts, packed, dq, B, want_input_grad=True)
            acc += gx.view_as(xn) * (1.0 / steps)
        return acc * (xn - black)

    ig = _alternate({"host_loop_full_backward": host_loop,
                     "integrated_gradients": lambda: model.integrated_gradients(xn, 3, steps=steps)}, max(1, args.reps // 2), args.rounds, warmup=1)
    a, b = host_loop().double().flatten(), model.integrated_gradients(xn, 3, steps=steps).double().flatten()
    ig.update(batch=B, steps=steps, max_batch=args.max_batch, host_over_engine=ig["ms_median"]["host_loop_full_backward"] / ig["ms_median"]["integrated_gradients"],
              cosine_host_vs_engine=float((a @ b) / (a.norm() * b.norm())))

    out = {"dtype": "bf16", "reps_per_window": args.reps, "rounds": args.rounds, "backward": backward, "integrated_gradients": ig,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
