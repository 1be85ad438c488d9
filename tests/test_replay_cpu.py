"""Prioritized experience replay without a GPU: the config keys, the workspace size of the C ABI, run_train's refusals (raised
before any device work) and the invariants of the numpy oracle the GPU tests compare the kernels against."""
import numpy as np
import pytest

import per_oracle


def test_config_keys_defaults_merge_and_types(tmp_path):
    from video_dqn_amd.config import get_cfg_defaults
    c = get_cfg_defaults()
    assert c.PRIORITIZED_REPLAY is False and c.PER_ALPHA == 0.6 and c.PER_BETA == 0.4
    f = tmp_path / "config.yml"
    f.write_text("PRIORITIZED_REPLAY: True\nPER_ALPHA: 1\nPER_BETA: 0.5\n")
    c.merge_from_file(str(f))
    assert c.PRIORITIZED_REPLAY is True and c.PER_ALPHA == 1.0 and isinstance(c.PER_ALPHA, float) and c.PER_BETA == 0.5
    for bad in ("PRIORITIZED_REPLAY: 'yes'\n", "PER_ALPHA: 'high'\n", "PER_BETA: True\n"):
        f.write_text(bad)
        with pytest.raises(ValueError, match="Type mismatch"):
            get_cfg_defaults().merge_from_file(str(f))


def test_per_workspace_bytes():
    from video_dqn_amd import _lib
    lib = _lib.load()
    for n in (1, 31, 32, 2047, 2048, 2049, 100003, 1000000):
        seg, chunk = -(-n // 32), -(-n // 2048)
        assert lib.vdqn_per_workspace_bytes(n) == -(-seg * 8 // 256) * 256 + -(-chunk * 8 // 256) * 256
    for n in (0, -1, 4096 * 2048 + 1):
        assert lib.vdqn_per_workspace_bytes(n) == -1


def _cfg(tmp_path, **keys):
    from video_dqn_amd.config import get_cfg_defaults
    c = get_cfg_defaults()
    c.PRIORITIZED_REPLAY = True
    for k, v in keys.items():
        c[k] = v
    c.folder = str(tmp_path)
    c.device = "cuda"
    return c


@pytest.mark.parametrize("keys,reason", [
    (dict(TRAIN_ON_GROUND_TRUTH=True), "TRAIN_ON_GROUND_TRUTH"),
    (dict(SYNTHETIC_DATA=True), "SYNTHETIC_DATA"),
    (dict(DATASET="synthetic"), "SYNTHETIC_DATA"),
    (dict(DATASET="FEATHER"), "feather\\+JPEG"),
    (dict(DATASET="SHARDS", DEVICE_RESIDENT_DATA="off"), "DEVICE_RESIDENT_DATA is 'off'"),
    (dict(DATASET="SHARDS", PER_ALPHA=-0.5), "PER_ALPHA must be >= 0"),
    (dict(DATASET="SHARDS", PER_BETA=1.5), "PER_BETA must be in"),
    (dict(DATASET="SHARDS", BATCH_SIZE=5000), "at most 4096 samples per update"),
], ids=["ground_truth", "synthetic", "dataset_synthetic", "feather_jpeg", "resident_off", "alpha", "beta", "global_batch"])
def test_run_train_refuses_before_device_work(tmp_path, monkeypatch, keys, reason):
    import torch
    from test_shards_cpu import _synthetic_shards
    from video_dqn_amd import trainer
    shards = str(tmp_path / "shards")
    _synthetic_shards(shards)
    (tmp_path / "data.feather").write_bytes(b"")
    keys = {k: (shards if v == "SHARDS" else str(tmp_path / "data.feather") if v == "FEATHER" else v) for k, v in keys.items()}

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(torch.cuda, "mem_get_info", no_device)
    monkeypatch.setattr(trainer, "build_model", no_device)
    with pytest.raises(ValueError, match=reason):
        trainer.run_train(_cfg(tmp_path, **keys), log=lambda *a: None)


def test_run_train_refuses_a_dataset_that_does_not_fit_in_hbm(tmp_path, monkeypatch):
    """The HBM-fit refusal: the frames plus the headroom against the free memory the device reports, before any upload."""
    import torch
    from test_shards_cpu import _synthetic_shards
    from video_dqn_amd import trainer
    shards = str(tmp_path / "shards")
    _synthetic_shards(shards)

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (8 << 30, 288 << 30))
    monkeypatch.setattr(trainer, "build_model", no_device)
    for resident in ("auto", "on"):
        with pytest.raises(ValueError, match="do not fit in 8.0 GiB of free HBM"):
            trainer.run_train(_cfg(tmp_path, DATASET=shards, DEVICE_RESIDENT_DATA=resident), log=lambda *a: None)


def test_oracle_uniform_priorities_one_index_per_stratum():
    for n, G in ((256, 256), (1000, 64), (4096, 512), (100003, 256)):
        idx, w = per_oracle.sample(np.ones(n, np.float32), G, seed=3, step=7, beta=0.4)
        lo = np.floor(np.arange(G) * n / G).astype(np.int64)
        hi = np.ceil((np.arange(G) + 1) * n / G).astype(np.int64)
        assert np.all(idx >= lo) and np.all(idx < hi), (n, G)
        assert np.all(np.diff(idx) > 0)
        assert np.all(w == 1.0)


def test_oracle_never_draws_zero_priority_and_clamps():
    rng = np.random.default_rng(0)
    p = np.where(rng.random(5000) < 0.7, 0.0, rng.random(5000)).astype(np.float32)
    idx, _ = per_oracle.sample(p, 512, seed=1, step=2, beta=0.4)
    assert np.all(p[idx] > 0)
    one = np.zeros(3000, np.float32)
    one[2999] = 5.0
    idx, w = per_oracle.sample(one, 256, seed=9, step=1, beta=0.7)
    assert np.all(idx == 2999) and np.all(w == 1.0)


def test_oracle_update_duplicate_rule():
    p = np.ones(10, np.float32)
    idx = np.array([3, 5, 3, 7, 3])
    err = np.array([0.1, 0.2, 0.3, 0.4, 0.5], np.float32)
    out = per_oracle.update(p, idx, err, 0.6)
    assert out[3] == np.float32((0.5 + 1e-6) ** 0.6)  # the largest j of index 3
    assert out[5] == np.float32((np.float64(np.float32(0.2)) + 1e-6) ** 0.6)
    assert np.all(out[[0, 1, 2, 4, 6, 8, 9]] == 1.0)
    assert np.all(per_oracle.update(p, idx, err, 0.0) == 1.0)


def test_beta_schedule():
    from video_dqn_amd.replay import beta_at
    for f in (beta_at, per_oracle.beta_at):
        assert f(0.4, 0, 1000) == 0.4
        assert abs(f(0.4, 500, 1000) - 0.7) < 1e-15
        assert f(0.4, 1000, 1000) == 1.0 and f(0.4, 5000, 1000) == 1.0


def test_error_exchange_sums_the_slices_over_gloo(tmp_path):
    """dist.BucketAllReduce.launch_errors + finish on CPU tensors: every rank ends with the global [G] error vector."""
    import torch.multiprocessing as mp
    mp.spawn(_exchange_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = (np.load(tmp_path / f"err{r}.npy") for r in range(2))
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, np.arange(8, dtype=np.float32) + 1)


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _exchange_worker(rank, world, port, out_dir):
    import os
    import torch
    import torch.distributed as dist
    from video_dqn_amd.dist import BucketAllReduce
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    err = torch.zeros(8)
    err[rank * 4:(rank + 1) * 4] = torch.arange(rank * 4, (rank + 1) * 4, dtype=torch.float32) + 1
    comm = BucketAllReduce(world)
    comm.launch_errors(err)
    comm.finish()
    np.save(os.path.join(out_dir, f"err{rank}.npy"), err.numpy())
    dist.barrier()
    dist.destroy_process_group()
