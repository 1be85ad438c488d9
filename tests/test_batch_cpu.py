"""The batch record (video_dqn_amd.shards.Batch): every combination of prioritized replay, n-step walker and return table through
DeviceFrameStore.batches / prioritized_batches on the CPU, with duck-typed stand-ins for the three helpers that launch HIP kernels."""
import itertools

import pytest
import torch

N, B, SEED = 37, 4, 11
OPTIONAL = ("weight", "discount", "mc_return")


class _Walker:
    """NStepWalker's interface: walk(idx) -> (rew_n, term_n, disc, last_row, steps), buffers of its own, last_row != idx."""

    def __init__(self):
        self.rew_n, self.term_n, self.disc = torch.full((B, 5), 7.5), torch.full((B, 5), 0.25), torch.full((B,), 0.9)
        self.last_row = None

    def walk(self, idx):
        self.last_row = (idx + 3) % N
        return self.rew_n, self.term_n, self.disc, self.last_row, torch.full((B,), 2)


class _Returns:
    G = torch.arange(N * 5).view(N, 5).float()


class _Sampler:
    """PrioritizedSampler's interface: .n and sample(step) -> (idx, weight)."""
    n = N

    def __init__(self):
        self.drawn = []

    def sample(self, step):
        idx = (torch.arange(B) * 5 + 2 * step) % N
        self.drawn.append((step, idx, torch.arange(B).float() + step))
        return self.drawn[-1][1:]


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    from test_shards_cpu import _synthetic_shards
    from video_dqn_amd.shards import DeviceFrameStore
    root = str(tmp_path_factory.mktemp("batch") / "shards")
    _synthetic_shards(root)  # 37 samples, 24 frames
    return DeviceFrameStore(root, "cpu", inverse_actions=True)


@pytest.mark.parametrize("per,nstep,mc", list(itertools.product((False, True), repeat=3)))
def test_every_source_combination_yields_the_named_batch(store, per, nstep, mc):
    from video_dqn_amd.shards import Batch
    walker, returns, sampler = (_Walker() if nstep else None), (_Returns() if mc else None), (_Sampler() if per else None)
    if per:
        it = store.prioritized_batches(sampler, 5, walker=walker, returns=returns)
    else:
        it = store.batches(B, SEED, walker=walker, returns=returns)
        perm = torch.randperm(N, generator=torch.Generator(device="cpu").manual_seed(SEED))
    for k in range(3):
        batch = next(it)
        if per:
            step, idx, weight = sampler.drawn[-1]
            assert step == 5 + k + 1 and len(sampler.drawn) == k + 1
        else:
            idx = perm[B * k:B * (k + 1)]
        assert isinstance(batch, Batch) and len(batch) == 11 and Batch._fields[8:] == OPTIONAL and len(batch[:]) == 8
        assert [f for f in OPTIONAL if getattr(batch, f) is not None] == [f for f, on in zip(OPTIONAL, (per, nstep, mc)) if on]
        sel = lambda table, rows: store.frames.index_select(0, table.index_select(0, rows).reshape(-1))  # noqa: E731
        assert torch.equal(batch.before, sel(store.before, idx)) and batch.src_kind == 0
        assert torch.equal(batch.act, store.act[idx]) and torch.equal(batch.valid, store.valid[idx])
        assert torch.equal(torch.nan_to_num(batch.gt, nan=-7.0), torch.nan_to_num(store.gt[idx], nan=-7.0))
        if nstep:
            assert not torch.equal(walker.last_row, idx)
            assert torch.equal(batch.after, sel(store.after, walker.last_row)) and not torch.equal(batch.after, sel(store.after, idx))
            assert batch.rew is walker.rew_n and batch.term is walker.term_n and batch.discount is walker.disc
        else:
            direct = (sel(store.before, idx), sel(store.after, idx), 0, store.act.index_select(0, idx), store.rew.index_select(0, idx),
                      store.term.index_select(0, idx), store.valid.index_select(0, idx), store.gt.index_select(0, idx))
            for x, y in zip(tuple(batch[:8]), direct):
                assert x == y if isinstance(y, int) else (x.dtype == y.dtype and x.shape == y.shape and
                                                          torch.equal(torch.nan_to_num(x.float(), nan=-7.0), torch.nan_to_num(y.float(), nan=-7.0)))
        if mc:
            assert torch.equal(batch.mc_return, _Returns.G[idx]) and batch.mc_return.shape == (B, 5)  # the SAMPLED rows, walker or not
        if per:
            assert batch.weight is weight


def test_to_device_batch_yields_the_named_batch():
    """The loader path's host batch (the datasets' 7-tuple) through trainer._to_device_batch: a Batch with the optional fields None."""
    from video_dqn_amd.shards import Batch
    from video_dqn_amd.trainer import _to_device_batch
    frames = torch.zeros(B, 224, 224, 3, dtype=torch.uint8)
    batch = _to_device_batch((frames, frames.clone(), torch.zeros(B, dtype=torch.int64), torch.ones(B, 5), torch.zeros(B, 5), torch.full((B,), float("nan")),
                              torch.ones(B, 5)), "cpu")
    assert isinstance(batch, Batch) and batch.weight is batch.discount is batch.mc_return is None and batch.src_kind == 0
    assert batch.gt.shape == (B, 5)


def test_an_index_or_a_slice_reads_the_eight_batch_tensors_alone():
    """Readers written for the former 8-tuple (`item[3:]`, `item[-1]`) see what they saw; the optional fields are read by name, and
    `_replace` and iteration still carry all eleven."""
    from video_dqn_amd.shards import Batch
    batch = Batch(*"abcdefgh")._replace(weight="w", mc_return="G")
    assert batch[3:] == tuple("defgh") and batch[:8] == batch[:] == tuple("abcdefgh") and batch[-1] == "h" and batch[8:] == ()
    assert (batch.weight, batch.discount, batch.mc_return) == ("w", None, "G") and tuple(batch) == tuple("abcdefgh") + ("w", None, "G")
    with pytest.raises(IndexError):
        batch[8]


def test_run_train_refuses_a_learning_rate_that_is_no_number_before_device_work(tmp_path, monkeypatch):
    """With an LR schedule on, LEARNING_RATE is converted where the checks run: behind check_mc and in front of the prioritized-replay
    check (its PER_ALPHA is wrong here too, and is not what is reported), before the dataset is opened or the model built."""
    from test_shards_cpu import _synthetic_shards
    from video_dqn_amd import trainer
    from video_dqn_amd.config import get_cfg_defaults
    shards = str(tmp_path / "shards")
    _synthetic_shards(shards)
    c = get_cfg_defaults()
    c.DATASET, c.LR_WARMUP_STEPS, c.LEARNING_RATE, c.PRIORITIZED_REPLAY, c.PER_ALPHA = shards, 10, "fast", True, -1.0
    c.folder, c.device = str(tmp_path), "cuda"

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(torch.cuda, "mem_get_info", no_device)
    monkeypatch.setattr(torch.cuda, "current_stream", no_device)
    monkeypatch.setattr(torch, "manual_seed", no_device)
    monkeypatch.setattr(trainer, "build_model", no_device)
    monkeypatch.setattr(trainer, "ShardDataset", no_device)
    with pytest.raises(ValueError, match="could not convert string to float: 'fast'"):
        trainer.run_train(c, log=lambda *a: None)
