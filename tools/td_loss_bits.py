"""Every output of the three TD-loss entries (vdqn_td_loss, vdqn_td_loss_weighted, vdqn_td_loss_cql) as .npy files, to compare two
builds of the library byte for byte:

    VDQN_LIB=<variant> python tools/td_loss_bits.py DIR_A        (one process per library: the variant is chosen at import)
    python tools/td_loss_bits.py DIR_B
    python tools/td_loss_bits.py --compare DIR_A DIR_B           (no GPU; exit status 1 unless every array is equal)

Cases: {f32, bf16} x {l2, huber} x {valid, none} x the four (linear, clip_rect, gamma) options of the tests x five shapes (one wave
of one block, a partly filled second block, no padding columns, exactly one block, the tests' 96 x 64), deterministic = 1 (the
one launch shape whose loss has a fixed order).  Q(s) is scaled by 2.5 so that both Huber branches occur; the weighted and the CQL
entry get non-unit weights.  Per case and entry: loss, dq (as stored, bf16 included), dq_f32, q_copy, and err / penalty where the
entry has them."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

SHAPES = [(1, 64), (5, 64), (17, 15), (16, 16), (96, 64)]
TARGETS = [(0, 1, 0.9), (1, 1, 0.9), (0, 0, 0.99), (1, 0, 0.5)]  # (linear, clip_rect, gamma)


def dump(out_dir):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from video_dqn_amd import _lib
    lib = _lib.load()
    dev = "cuda"
    os.makedirs(out_dir, exist_ok=True)
    st = torch.cuda.current_stream().cuda_stream
    n = 0
    for B, ldq in SHAPES:
        g = torch.Generator().manual_seed(1000 * B + ldq)
        q = [(torch.randn(B, ldq, generator=g) * 0.7).to(dev) for _ in range(3)]
        q[0] = q[0] * 2.5
        act = torch.randint(0, 3, (B,), generator=g).to(dev)
        rew = (torch.rand(B, 5, generator=g) < 0.3).float().to(dev)
        term = (torch.rand(B, 5, generator=g) < 0.2).float().to(dev)
        valid = (torch.rand(B, 5, generator=g) < 0.8).float().to(dev)
        w = (torch.rand(B, generator=g) * 0.9 + 0.1).to(dev)
        for dtype, dname in ((_lib.VDQN_F32, "f32"), (_lib.VDQN_BF16, "bf16")):
            for loss_kind in (0, 1):
                for use_valid in (0, 1):
                    for linear, clip_rect, gamma in TARGETS:
                        for entry in ("plain", "weighted", "cql"):
                            loss, pen = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
                            dq = torch.full((B, ldq), 7.0, dtype=torch.bfloat16 if dtype == _lib.VDQN_BF16 else torch.float32, device=dev)
                            dq32 = torch.full((B, ldq), 7.0, device=dev)
                            err = torch.full((B,), -1.0, device=dev)
                            qc = torch.full((B, 15), -7.0, device=dev)
                            a = _lib.TdArgs()
                            a.q_before, a.q_after_online, a.q_after_target = q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr()
                            a.act, a.rew, a.term, a.valid = act.data_ptr(), rew.data_ptr(), term.data_ptr(), valid.data_ptr() if use_valid else None
                            a.loss, a.dq, a.dq_f32, a.q_copy = loss.data_ptr(), dq.data_ptr(), dq32.data_ptr(), qc.data_ptr()
                            a.batch, a.n_cat, a.n_act, a.ldq = B, 5, 3, ldq
                            a.gamma, a.inv_count = gamma, 1.0 / (5 * B)
                            a.clip_rect, a.linear, a.use_valid, a.dtype, a.loss_kind, a.deterministic = clip_rect, linear, use_valid, dtype, loss_kind, 1
                            if entry == "plain":
                                _lib.check(lib.vdqn_td_loss(C.byref(a), st), "vdqn_td_loss")
                            elif entry == "weighted":
                                _lib.check(lib.vdqn_td_loss_weighted(C.byref(a), w.data_ptr(), err.data_ptr(), st), "vdqn_td_loss_weighted")
                            else:
                                _lib.check(lib.vdqn_td_loss_cql(C.byref(a), w.data_ptr(), err.data_ptr(), 1.5, pen.data_ptr(), st), "vdqn_td_loss_cql")
                            torch.cuda.synchronize()
                            tag = f"B{B}_ld{ldq}_{dname}_k{loss_kind}_v{use_valid}_l{linear}c{clip_rect}g{gamma}_{entry}"
                            outs = {"loss": loss, "dq": dq.view(torch.int16) if dtype == _lib.VDQN_BF16 else dq, "dq_f32": dq32, "q_copy": qc}
                            if entry != "plain":
                                outs["err"] = err
                            if entry == "cql":
                                outs["penalty"] = pen
                            for name, t in outs.items():
                                np.save(os.path.join(out_dir, f"{tag}_{name}.npy"), t.cpu().numpy())
                                n += 1
    print(f"{n} arrays written to {out_dir} from {_lib.LIB_PATH}")


def compare(dir_a, dir_b):
    names_a, names_b = sorted(os.listdir(dir_a)), sorted(os.listdir(dir_b))
    if names_a != names_b or not names_a:
        print(f"the directories hold different files ({len(names_a)} / {len(names_b)})")
        return 1
    bad, nbytes = [], 0
    for name in names_a:
        x, y = np.load(os.path.join(dir_a, name)), np.load(os.path.join(dir_b, name))
        nbytes += x.nbytes
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(name)
    print(f"{len(names_a)} arrays, {nbytes} bytes: {len(names_a) - len(bad)} equal byte for byte, {len(bad)} differ")
    for name in bad[:20]:
        print("  differs:", name)
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("dirs", nargs="+")
    args = ap.parse_args()
    if args.compare:
        if len(args.dirs) != 2:
            ap.error("--compare takes two directories")
        sys.exit(compare(*args.dirs))
    dump(args.dirs[0])
