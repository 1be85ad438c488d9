#!/usr/bin/env python
"""Record of the engine's layouts: the parameter table, the packed-weight size, the stage ranges and the two workspace layouts
(activations, backward) for every architecture / dtype / frame count / deterministic flag / batch the layout code branches on.

    python tests/golden/make_engine_layout.py --tree <checkout of the commit to record> --out tests/golden/engine_layout.json

The fixture is written from the library of the commit BEFORE a change to the layout code (a separate checkout, built there),
never from the tree under test; tests/test_engine_layout_cpu.py recomputes the same record from the tree under test.  Needs no
GPU: the layout entries are host arithmetic.

Per combination: [packed_bytes, [stage 0 begin, end, stage 1 begin, end, stage 2 begin, end], acts_bytes(n), bwd_bytes(n),
SHA-256 of the sorted "name=value" lines of table_lines()].
"""
import argparse
import hashlib
import itertools
import json
import os
import sys

ARCHS = ("extra_capacity", "basic")
DTYPES = ("bf16", "f32", "bf16x3")
FRAMES = (1, 4)
DETERMINISTIC = (0, 1)
BATCHES = (1, 3, 8, 33)

_IDX = [str(i) for i in range(8)]
ACT_NAMES = (["t_in", "c1", "pool", "idx", "f8", "l0", "l1", "q", "qf", "avg", "r_c1"]
             + [p + i for p in ("h", "o", "ds", "r_h", "r_o", "r_ds") for i in _IDX])
BWD_NAMES = (["dq", "g_l1", "g_l0", "g_f8", "g_pool", "g_c1", "g_avg"]
             + [p + i for p in ("g_o", "g_h", "dsg", "g_or", "g_dsr") for i in _IDX])


def key(arch, dtype, frames, det, n):
    return f"{arch}/{dtype}/F{frames}/det{det}/n{n}"


def table_lines(net, n):
    """Sorted name=value lines: the parameter table, and every workspace offset at n and 2 * n samples."""
    lib, h = net.lib, net.handle
    lines = [f"param:{s.name}={s.offset},{s.numel},{'x'.join(map(str, s.shape))},{s.kind},{s.param_id},{s.stage}" for s in net.slots.values()]
    layers = [s.name[:-len(".weight")] for s in net.slots.values() if len(s.shape) >= 2]
    for m in (n, 2 * n):
        lines += [f"act:{m}:{nm}={lib.vdqn_net_act_offset(h, m, nm.encode())}" for nm in ACT_NAMES]
        lines += [f"bwd:{m}:{nm}={lib.vdqn_net_bwd_offset(h, m, nm.encode())}" for nm in BWD_NAMES]
        lines += [f"bwd:{m}:{k}:{ly}={lib.vdqn_net_bwd_offset(h, m, f'{k}:{ly}'.encode())}" for ly in layers for k in ("dw", "db")]
    return sorted(lines)


def record(arch, dtype, frames, det, n):
    from video_dqn_amd.engine import NetEngine
    net = NetEngine(3, 5, frames, arch == "extra_capacity", dtype, 128, device="cpu", deterministic=bool(det))
    stages = [int(v) for st in range(3) for v in net.stage_range(st)]
    lines = table_lines(net, n)
    sha = hashlib.sha256("\n".join(lines).encode()).hexdigest()
    return [int(net.packed_bytes), stages, int(net.acts_bytes(n)), int(net.bwd_bytes(n)), sha], lines


def all_records():
    out = {}
    for arch, dtype, frames, det, n in itertools.product(ARCHS, DTYPES, FRAMES, DETERMINISTIC, BATCHES):
        out[key(arch, dtype, frames, det, n)] = record(arch, dtype, frames, det, n)[0]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True, help="root of the checkout whose built library is recorded")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import video_dqn_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(video_dqn_amd.__file__))) == os.path.abspath(a.tree), video_dqn_amd.__file__
    recs = all_records()
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in recs.items()) + "\n}\n")
    print(f"{len(recs)} combinations -> {a.out}")
