"""p, exp_avg, exp_avg_sq and the target after one and after two steps of the three Adam entries (vdqn_adam, vdqn_adam_scaled,
vdqn_adam_polyak) as .npy files, to compare two builds of the library:

    VDQN_LIB=<variant> python tools/adam_bits.py DIR_A           (one process per library: the variant is chosen at import)
    python tools/adam_bits.py DIR_B
    python tools/adam_bits.py --compare DIR_A DIR_B              (no GPU; exit status 1 unless all three conditions below hold)

Cases: the sizes of tests/test_gpu_polyak.py (SIZES + [PAST_THE_CAP]: every tail length, more than one block, a second pass of the
capped grid) and that file's _adam_state (moments that are not zero) x {vdqn_adam; vdqn_adam_scaled and vdqn_adam_polyak at unit
factors (coef NULL, weight_decay 0) and at coef 0.37, weight_decay 0.1; vdqn_adam_polyak at tau 0.005 and 0.5}.  The largest size
writes 17 MB per array, about 0.9 GB per directory.

--compare is written for a build whose scalar tail loop (the last n % 4 elements of a range) differs from the other's while the
float4 loop is the same arithmetic.  It demands
  1. every array equal at all positions below n - n % 4,
  2. after one step, exp_avg equal everywhere,
  3. after one step, exp_avg_sq within 1 ulp at the last n % 4 positions,
and prints, per condition, how many arrays miss it and the largest distance in ulps."""
import argparse
import os
import re
import sys

import numpy as np

SIZES = [1, 2, 3, 5, 255, 256, 257, 1025, 100003, 4096 * 256 * 4 + 5]
NAMES = ("p", "exp_avg", "exp_avg_sq", "target")


def adam_state(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, n).astype(np.float32)
    g = rng.uniform(-1e-3, 1e-3, n).astype(np.float32)
    g[::7] = 0.0
    m = rng.uniform(-1e-3, 1e-3, n).astype(np.float32)
    v = rng.uniform(0, 1e-6, n).astype(np.float32)
    t = (p + 0.01 * rng.standard_normal(n)).astype(np.float32)
    return p, g, m, v, t


def dump(out_dir):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from video_dqn_amd import _lib, ops
    dev = "cuda"
    os.makedirs(out_dir, exist_ok=True)
    coef = torch.full((1,), 0.37, dtype=torch.float32, device=dev)
    factors = {"unit": dict(weight_decay=0.0, coef=None), "scaled": dict(weight_decay=0.1, coef=coef)}
    cases = [("adam", None, None)] + [("adam_scaled", f, None) for f in factors] + [("adam_polyak", f, tau) for f in factors for tau in (0.005, 0.5)]
    count = 0
    for n in SIZES:
        host = [torch.from_numpy(x).to(dev) for x in adam_state(n, 3 * n + 1)]
        for entry, f, tau in cases:
            p, g, m, v, t = (x.clone() for x in host)
            for step in (1, 2):
                if entry == "adam":
                    ops.adam(p, g, m, v, step, 1e-3)
                elif entry == "adam_scaled":
                    ops.adam_scaled(p, g, m, v, step, 1e-3, **factors[f])
                else:
                    ops.adam_polyak(p, g, m, v, t, tau, step, 1e-3, **factors[f])
                torch.cuda.synchronize()
                tag = f"n{n}_{entry}" + (f"_{f}" if f else "") + (f"_tau{tau}" if tau else "") + f"_step{step}"
                for name, x in zip(NAMES, (p, m, v, t)):
                    if name != "target" or entry == "adam_polyak":
                        np.save(os.path.join(out_dir, f"{tag}_{name}.npy"), x.cpu().numpy())
                        count += 1
    print(f"{count} arrays written to {out_dir} from {_lib.LIB_PATH}")


def ulps(x, y):
    """Largest distance of two f32 arrays in units in the last place (0 for no elements)."""
    def ordered(a):
        i = a.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(ordered(x) - ordered(y)).max()) if x.size else 0


def compare(dir_a, dir_b):
    names_a, names_b = sorted(os.listdir(dir_a)), sorted(os.listdir(dir_b))
    if names_a != names_b or not names_a:
        print(f"the directories hold different files ({len(names_a)} / {len(names_b)})")
        return 1
    checks = {"1. equal below n - n % 4": [], "2. step 1: exp_avg equal everywhere": [], "3. step 1: exp_avg_sq within 1 ulp in the tail": []}
    other_tail, nbytes = [], 0
    for name in names_a:
        x, y = np.load(os.path.join(dir_a, name)), np.load(os.path.join(dir_b, name))
        if x.dtype != np.float32 or y.dtype != np.float32 or x.shape != y.shape:
            print("not two f32 arrays of one shape:", name)
            return 1
        nbytes += x.nbytes
        n, step, what = int(re.match(r"n(\d+)_", name).group(1)), int(re.search(r"_step(\d)_", name).group(1)), name.split("_step")[1][2:-4]
        body = n - n % 4
        d_body, d_tail = ulps(x[:body], y[:body]), ulps(x[body:], y[body:])
        if d_body:
            checks["1. equal below n - n % 4"].append((d_body, name))
        if step == 1 and what == "exp_avg" and (d_body or d_tail):
            checks["2. step 1: exp_avg equal everywhere"].append((max(d_body, d_tail), name))
        if step == 1 and what == "exp_avg_sq" and d_tail > 1:
            checks["3. step 1: exp_avg_sq within 1 ulp in the tail"].append((d_tail, name))
        if d_tail:
            other_tail.append((d_tail, name))
    print(f"{len(names_a)} arrays, {nbytes} bytes")
    for title, bad in checks.items():
        print(f"{title}: {'holds' if not bad else f'{len(bad)} arrays miss it, worst {max(bad)[0]} ulps ({max(bad)[1]})'}")
    print(f"arrays whose last n % 4 elements differ at all: {len(other_tail)}" + (f", worst {max(other_tail)[0]} ulps ({max(other_tail)[1]})" if other_tail else ""))
    return 1 if any(checks.values()) else 0


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
