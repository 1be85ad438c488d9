#!/usr/bin/env python
"""The bits of a few deterministic updates in each way of forming the loss — plain TD, CQL, CQL + return floor + calibration, IQL,
distributional, BCQ — written as raw files to --out DIR: loss, the mode's statistics, the flat gradient and the parameters.  Run it
in two trees on one GPU and compare the directories with `cmp`: a change that only rewires the path from the arguments to the
loss launch leaves every file identical.  Uses only arguments every tree since the BCQ head has."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_dqn_amd import synth  # noqa: E402
from video_dqn_amd.engine import NetEngine, TDStepper  # noqa: E402

# mode -> (NetEngine arguments, TDStepper arguments, the stepper's statistics to keep)
MODES = {
    "plain": ({}, {}, ()),
    "cql": ({}, dict(cql_alpha=1.0), ("cql_penalty",)),
    "calql": ({}, dict(cql_alpha=1.0, mc_floor=True, cql_calibrated=True), ("cql_penalty", "mc_stats")),
    "iql": (dict(value_head=True), dict(iql_expectile=0.7), ("iql_stats",)),
    "dist": (dict(spread_head=True), dict(distributional=True), ("dist_stats",)),
    "bcq": (dict(policy_head=True), dict(bcq_threshold=0.3), ("bcq_stats",)),
}


def build(mode, dtype, B, seed=7):
    """-> (net, stepper) of `mode`: deterministic engine, synthetic weights, the extra head's rows from a seeded generator."""
    net_kw, step_kw, _ = MODES[mode]
    net = NetEngine(3, 5, 1, True, dtype, 2 * B, deterministic=True, **net_kw)
    net.load_tensors(synth.make_state_dict(seed))
    g = torch.Generator().manual_seed(seed + 1)
    for name in net.head_keys:
        v = net.view(name)
        v.copy_((0.05 * torch.randn(v.shape, generator=g)).to(v.device))
    net.mark_dirty()
    return net, TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, **step_kw)


def inputs(mode, B, dev, seed=1234):
    """-> (positional arguments of TDStepper.step, its keyword arguments): seeded frames, actions, rewards, terminals."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    before = torch.randint(0, 256, (B, 1, 224, 224, 3), dtype=torch.uint8, device=dev, generator=g)
    after = torch.randint(0, 256, (B, 1, 224, 224, 3), dtype=torch.uint8, device=dev, generator=g)
    act = torch.randint(0, 3, (B,), dtype=torch.int64, device=dev, generator=g)
    rew = (torch.rand((B, 5), device=dev, generator=g) < 0.3).float()
    term = (torch.rand((B, 5), device=dev, generator=g) < 0.2).float()
    kw = {}
    if mode == "calql":  # returns on both sides of the targets: the floor raises some, the calibration caps some
        kw["mc_return"] = 2.0 * torch.rand((B, 5), device=dev, generator=g) - 0.5
    return (before, after, 0, act, rew, term), kw


def run(mode, dtype, B, updates):
    """-> {file stem: tensor} after `updates` updates."""
    net, stp = build(mode, dtype, B)
    args, kw = inputs(mode, B, net.device)
    for _ in range(updates):
        loss = stp.step(*args, **kw)
    torch.cuda.synchronize()
    out = {"loss": loss, "grads": stp.grads, "params": net.params}
    out.update({name: getattr(stp, name) for name in MODES[mode][2]})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--updates", type=int, default=3)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for dtype in ("f32", "bf16"):
        for mode in MODES:
            for stem, t in run(mode, dtype, a.batch, a.updates).items():
                t.detach().cpu().contiguous().numpy().tofile(os.path.join(a.out, f"{mode}_{dtype}_{stem}.bin"))
            print(f"{mode} {dtype}: written", flush=True)


if __name__ == "__main__":
    main()
