"""Cost of the conservative Q-learning penalty in one process: alternating timed windows of TD updates at batch B (bf16) through a
TDStepper with cql_alpha = 0 — the update as it is without the feature, the baseline — and one with cql_alpha = 1 on the same
engine (as tools/ab_inproc.py and tools/bench_optim.py alternate their variants), then the device time of the loss launch of
each (launch profiler, windows of their own), and of the loss kernels alone in their one-block deterministic mode.

    python tools/bench_cql.py [--batch 256] [--steps 30] [--rounds 6] [--out profiles/cql_bench.json]

The baseline is never a separate run: two processes differ by more than the effect looked for."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

KERNELS = ("td_loss", "td_loss_w", "td_loss_cql")


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
    net = NetEngine(3, 5, 1, True, "bf16", 2 * B, device=dev)
    net.load_tensors(synth.make_state_dict(7))
    steppers = {"alpha0": TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, cql_alpha=0.0),
                "alpha1": TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, cql_alpha=1.0)}
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
    kernels = {}
    for m in modes:
        _lib.profile_enable(True)
        window(m, args.steps)
        prof = _lib.profile_collect()
        _lib.profile_enable(False)
        kernels[m] = {name: dict(launches_per_update=e["launches"] / args.steps, us_per_update=1e3 * e["ms"] / args.steps)
                      for name, e in prof.items() if name in KERNELS}
    penalty = steppers["alpha1"].cql_penalty.item()

    # the loss kernels alone, multi-block and in the one-block deterministic mode, on B x 64 random Q rows
    lib = _lib.load()
    g = torch.Generator().manual_seed(1)
    q = [(torch.randn(B, 64, generator=g) * 0.7).to(dev) for _ in range(3)]
    a_ = torch.randint(0, 3, (B,), generator=g).to(dev)
    r_ = (torch.rand(B, 5, generator=g) < 0.3).float().to(dev)
    t_ = (torch.rand(B, 5, generator=g) < 0.2).float().to(dev)
    w_ = (torch.rand(B, generator=g) * 0.9 + 0.1).to(dev)
    loss, pen = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    dq = torch.empty(B, 64, dtype=torch.bfloat16, device=dev)
    ta = _lib.TdArgs()
    ta.q_before, ta.q_after_online, ta.q_after_target = q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr()
    ta.act, ta.rew, ta.term, ta.loss, ta.dq = a_.data_ptr(), r_.data_ptr(), t_.data_ptr(), loss.data_ptr(), dq.data_ptr()
    ta.batch, ta.n_cat, ta.n_act, ta.ldq = B, 5, 3, 64
    ta.gamma, ta.inv_count, ta.clip_rect, ta.dtype = 0.99, 1.0 / (5 * B), 1, _lib.VDQN_BF16
    st = torch.cuda.current_stream().cuda_stream
    alone = {}
    for det in (0, 1):
        ta.deterministic = det
        for _ in range(2):  # (the first pass warms up)
            _lib.profile_enable(True)
            for _ in range(50):
                _lib.check(lib.vdqn_td_loss(C.byref(ta), st), "vdqn_td_loss")
                _lib.check(lib.vdqn_td_loss_weighted(C.byref(ta), w_.data_ptr(), None, st), "vdqn_td_loss_weighted")
                _lib.check(lib.vdqn_td_loss_cql(C.byref(ta), None, None, 1.0, pen.data_ptr(), st), "vdqn_td_loss_cql")
            prof = _lib.profile_collect()
            _lib.profile_enable(False)
        alone["deterministic" if det else "default"] = {name: 1e3 * e["ms"] / e["launches"] for name, e in prof.items() if name in KERNELS}

    med = {m: _median(v) for m, v in res.items()}
    out = {"batch": B, "dtype": "bf16", "steps_per_window": args.steps, "rounds": args.rounds,
           "ms_per_update": res, "ms_per_update_median": med,
           "window_spread": {m: (max(v) - min(v)) / med[m] for m, v in res.items()},
           "alpha1_over_alpha0": med["alpha1"] / med["alpha0"] - 1,
           "loss_launch_us_per_update": kernels, "loss_kernel_alone_us": alone, "last_cql_penalty": penalty,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
