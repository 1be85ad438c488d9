#!/usr/bin/env python
"""What `video_dqn_amd.trainer.run_train` logs, writes and leaves behind, as text that two trees can be compared by:

    python tools/trainer_trace.py [--tree DIR] [--work DIR] > trace.txt

runs four small deterministic f32 configurations at BATCH_SIZE 4 on synthetic 96-row shards — the generated-tuple loader path, the
HBM-resident store, the streamed shards, and every optional key at once (prioritized replay, N_STEP 3, both Monte-Carlo keys, CQL, shift
+ mirror + colour jitter, soft targets, clipping, validation; 100 updates, so that every scalar tag is written once; the others run
12) — and prints, per configuration, the captured log lines, the rows of scalars.jsonl, the returned running loss and the SHA-256 of
params, exp_avg, exp_avg_sq, loss, target_params and the priority table where they exist.  --tree DIR imports video_dqn_amd from DIR (a
checkout of another commit with its library built) in place of this tree; the output of the two must be identical line for line."""
import argparse
import contextlib
import hashlib
import io
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = ("PANORAMA: False\nLOSS_CLIP: 'rect'\nARCHITECTURE: 'extra_capacity'\nLEARNING_RATE: 0.0001\nGAMMA: 0.99\nUSE_INVERSE_ACTIONS: True\n"
        "CHECKPOINT_INTERVAL: 1000\nSEED: 4\nBATCH_SIZE: 4\nNUM_WORKERS: 0\nCOMPUTE_DTYPE: 'f32'\nDETERMINISTIC: True\nTARGET_UPDATE_INTERVAL: 3\n")
EVERYTHING = ("PRIORITIZED_REPLAY: True\nN_STEP: 3\nMC_RETURN_FLOOR: True\nCQL_CALIBRATED: True\nCQL_ALPHA: 1.0\nAUG_SHIFT_PAD: 4\nAUG_FLIP: True\n"
              "AUG_BRIGHTNESS: 0.2\nAUG_CONTRAST: 0.2\nAUG_SATURATION: 0.2\nTARGET_TAU: 0.01\nGRAD_CLIP_NORM: 10.0\nVAL_INTERVAL: 50\nVAL_BATCHES: 2\n")


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="the checkout video_dqn_amd is imported from")
    ap.add_argument("--work", default="/tmp/vdqn_trainer_trace", help="scratch directory (the same path for both trees: log lines name it)")
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.tree), ROOT]
    import torch
    from tools.bench_loader import make_shards
    import video_dqn_amd
    from video_dqn_amd.config import ExperimentConfig, JsonlWriter
    from video_dqn_amd.trainer import run_train
    assert os.path.dirname(os.path.dirname(os.path.abspath(video_dqn_amd.__file__))) == os.path.abspath(args.tree)
    shutil.rmtree(args.work, ignore_errors=True)
    shards = os.path.join(args.work, "shards")
    make_shards(shards, n_frames=24, shard_frames=8, n_samples=96)
    runs = (("synthetic_loader", 12, "DATASET: 'synthetic'\n"),
            ("resident", 12, f"DATASET: '{shards}'\nDEVICE_RESIDENT_DATA: 'on'\n"),
            ("streaming", 12, f"DATASET: '{shards}'\nDEVICE_RESIDENT_DATA: 'off'\n"),
            ("everything", 100, f"DATASET: '{shards}'\nDEVICE_RESIDENT_DATA: 'on'\nVAL_DATASET: '{shards}'\n" + EVERYTHING))
    for tag, steps, extra in runs:
        folder = os.path.join(args.work, tag)
        os.makedirs(folder)
        with open(os.path.join(folder, "config.yml"), "w") as f:
            f.write(BASE + f"NUM_STEPS: {steps}\n" + extra)
        cfg = ExperimentConfig(folder, device="cuda", tensorboard=True)
        if not isinstance(cfg.writer, JsonlWriter):
            raise SystemExit("this script reads scalars.jsonl: it needs the JsonlWriter stand-in (no tensorboard package)")
        logs = []
        with contextlib.redirect_stdout(io.StringIO()):  # (the progress line of every update)
            model, stepper, running = run_train(cfg, log=lambda *a: logs.append(" ".join(map(str, a))))
        torch.cuda.synchronize()
        cfg.writer.close()
        print(f"\n==== {tag}: {steps} updates, adam_step {stepper.adam_step}, running loss {running!r}")
        for line in logs:
            print("log    |", line)
        for row in open(os.path.join(cfg.log_dir, "scalars.jsonl")):
            print("scalar |", row.rstrip())
        tensors = {"params": model.engine.params, "exp_avg": stepper.exp_avg, "exp_avg_sq": stepper.exp_avg_sq, "loss": stepper.loss,
                   "target_params": stepper.target_params, "priorities": getattr(stepper.replay, "prio", None)}
        for name, t in tensors.items():
            if t is not None:
                print(f"sha256 | {name:14s} {sha(t)}")


if __name__ == "__main__":
    main()
