"""Rank program for tests/test_gpu_polyak.py: one rank of a two-rank gloo job on ONE device, B samples per rank, soft target updates
(target_tau) on the reduced gradient.  `run` is also what the test calls in-process for the one-process big batch.

    python polyak_two_ranks.py <rank> <world> <port> <out_dir> <per_rank> <tau>
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

LR, WARMUP, STEPS = 1e-4, 4, 2  # (the rates of optim_two_ranks.py: the bounds of its test are for these)


def lr_fn(t):
    from video_dqn_amd.optim import lr_at
    return lr_at(t, LR, WARMUP, "constant", 0.0, 100)


def run(B, world, rank, tau, hook=None):
    """STEPS updates of this rank's slice of the global batch -> dict of CPU tensors (params, target_params, loss per update)."""
    from video_dqn_amd import synth
    from video_dqn_amd.engine import NetEngine, TDStepper
    net = NetEngine(3, 5, 1, True, "f32", 2 * B, deterministic=True)
    net.load_tensors(synth.make_state_dict(7))
    stp = TDStepper(net, B, lr=LR, gamma=0.99, clip_rect=True, world_size=world, allreduce=hook, lr_fn=lr_fn, target_tau=tau)
    start = net.params.cpu().clone()
    for s in range(1, STEPS + 1):
        (tup, _) = synth.make_batch(200 + s, B * world, 1, structured=True, reward_p=0.3)
        lo, hi = rank * B, (rank + 1) * B
        stp.step(tup[0][lo:hi].contiguous().cuda(), tup[1][lo:hi].contiguous().cuda(), 1, tup[2][lo:hi].cuda(),
                 tup[3][lo:hi].float().cuda(), tup[4][lo:hi].float().cuda())
        torch.cuda.synchronize()
    return {"start": start, "params": net.params.cpu(), "target_params": None if stp.target_params is None else stp.target_params.cpu(),
            "trainable": net.trainable_numel}


if __name__ == "__main__":
    rank, world, port, out_dir, per_rank, tau = (int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], int(sys.argv[5]),
                                                 float(sys.argv[6]))
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", port
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)

    def through_host(t, stage=None):  # test transport (as tests/test_gpu_ddp.py): whatever gloo's GPU support is
        torch.cuda.synchronize()
        h = t.cpu()
        dist.all_reduce(h)
        t.copy_(h)

    out = run(per_rank, world, rank, tau, through_host)
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()
