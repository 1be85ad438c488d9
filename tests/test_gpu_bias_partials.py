"""dL/dbias and dL/dbeta of every layer against the gradient tensor the engine STORED for that layer's output.

The data-gradient kernels write per-tile column sums of what they store (vdqn_conv_args.colsum_part) and the unfold kernel adds
the entries up; csrc/engine_table.hip `part_info` is the one place that says where a layer's entries are and how many.  A
miscounted entry, a wrong stride or a missed parity class shows here as a missing or doubled block of rows.

After one TDStepper.forward_backward (no optimiser step) the stored tensors are read out of `stp.bwd` through
vdqn_net_bwd_offset and summed per column in float64.  The kernels add the same stored values in f32 in some order, and for any
order the error of an n-term f32 sum is at most gamma_(n-1) * sum|g| with gamma_(n-1) <= 1.01 * (n - 1) * 2^-24 while
n * 2^-24 < 0.01 (the largest n here is 33 * 56^2 = 103488).  So per channel

    |got - sum64| <= 1.01 * rows * 2^-24 * sum|g|  +  one f32 ulp of |sum64| (the final rounding)

with rows and sum|g| of that tensor and channel, and no relative tolerance on top.

Shapes: (B, F) = (3, 1): layer4 has 147 rows (two 128-row entries, the second ragged), layer3's g_o5 comes from a stride-2 data
gradient with 588 rows (four parity classes: 8 entries, 5 plain ones), the head is a single 32-row entry.  (2, 4): the features.8
grouping with F > 1 (25 * F groups in rows of 1600 * F).  (33, 1): the head gets two 32-row entries, the second holding one row,
and the stem's partials their largest row count; the same case once more in a child process with VDQN_SKINNY=0 (read once per
process), where the head goes through the generic kernels at 128 rows per entry."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__" and ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from video_dqn_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _state_dict(F):
    return synth.make_state_dict(7, num_frames=F)


def _stored_tensors(F):
    """gradient name -> (bwd workspace name, rows per sample, channels)"""
    out = {"top.2.bias": ("g_l1", 1, 256), "top.0.bias": ("g_l0", 1, 512), "features.8.bias": ("g_f8", F * 25, 64),
           "resnet.bn1.bias": ("g_pool", F * 56 * 56, 64), "top.4.bias": ("dq", 1, 64)}
    for b in range(8):
        L, K = b // 2 + 1, b % 2
        planes, sp = 64 << (b // 2), 56 >> (b // 2)
        out[f"resnet.layer{L}.{K}.bn2.bias"] = (f"g_o{b}", F * sp * sp, planes)
        if K == 0 and L > 1:
            out[f"resnet.layer{L}.{K}.downsample.1.bias"] = (f"g_o{b}", F * sp * sp, planes)
        out[f"resnet.layer{L}.{K}.bn1.bias"] = (f"g_h{b}", F * sp * sp, planes)
    return out


def check(B, F, dtype):
    from video_dqn_amd.engine import NetEngine, TDStepper
    net = NetEngine(3, 5, F, True, dtype, 2 * B)
    net.load_tensors(_state_dict(F))
    stp = TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True)
    (tup, _) = synth.make_batch(311, B, F, structured=True, reward_p=0.3)
    before, after, act, rew, term, gt, vm = tup
    stp.forward_backward(before.contiguous().to(DEV), after.contiguous().to(DEV), 1, act.to(DEV), rew.float().to(DEV), term.float().to(DEV))
    torch.cuda.synchronize()
    tdt, esz = (torch.bfloat16, 2) if dtype == "bf16" else (torch.float32, 4)
    bad = []
    for gname, (wname, rows_per_sample, ch) in _stored_tensors(F).items():
        rows = B * rows_per_sample
        off = net.lib.vdqn_net_bwd_offset(net.handle, B, wname.encode())
        assert off >= 0, wname
        g = stp.bwd[off:off + rows * ch * esz].view(tdt).view(rows, ch).double()
        s = net.slots[gname]
        got = stp.grads[s.offset:s.offset + s.numel].double().cpu().numpy()
        sum64 = g.sum(0).cpu().numpy()[:s.numel]
        sumabs = g.abs().sum(0).cpu().numpy()[:s.numel]
        bound = 1.01 * rows * 2.0 ** -24 * sumabs + np.spacing(np.abs(sum64).astype(np.float32)).astype(np.float64)
        err = np.abs(got - sum64)
        worst = int(np.argmax(err / bound))
        print(f"B={B} F={F} {dtype} {gname:40s} <- {wname:7s} [{rows}][{ch}]  max err {err.max():.3e}  "
              f"(nearest its bound, channel {worst}: err {err[worst]:.3e}, bound {bound[worst]:.3e}, |sum| {abs(sum64[worst]):.3e})")
        assert sumabs.max() > 0, f"{wname} is all zero: nothing was checked"
        if not (err <= bound).all():
            bad.append(gname)
    assert not bad, f"B={B} F={F} {dtype}: bias gradients off their stored tensors' column sums: {bad}"


@pytest.mark.parametrize("B,F,dtype", [(3, 1, "bf16"), (3, 1, "f32"), (2, 4, "bf16"), (2, 4, "f32"), (33, 1, "bf16")])
def test_bias_gradients_are_the_column_sums_of_the_stored_gradients(B, F, dtype):
    check(B, F, dtype)


def test_head_through_the_generic_kernels_in_a_child_process():
    """VDQN_SKINNY=0: the head's data gradients report 128 rows per entry instead of 32 (the other branch of the report)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "33", "1", "bf16"], env=dict(os.environ, VDQN_SKINNY="0"), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "child ok", r.stdout[-4000:]


if __name__ == "__main__":
    check(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3])
    print("child ok")
