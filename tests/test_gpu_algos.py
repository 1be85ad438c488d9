"""TDStepper's one `loss_stats` tensor in each way of forming the loss: which slots an update writes, that the named statistics are
views of it, and that two steppers built alike stay bit-identical.  (The raw entries against the operators, bit for bit:
test_gpu_iql / test_gpu_dist / test_gpu_bcq / test_gpu_cql / test_gpu_mcreturn.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 4  # the smallest batch at which the online pass over [s; s'] still holds both halves of more than one sample each
# mode -> (NetEngine arguments, TDStepper arguments, {statistics attribute: its slots of loss_stats})
MODES = {
    "plain": ({}, {}, {}),
    "cql": ({}, dict(cql_alpha=1.0), {"cql_penalty": (0, 1)}),
    "calql": ({}, dict(cql_alpha=1.0, mc_floor=True, cql_calibrated=True), {"cql_penalty": (0, 1), "mc_stats": (1, 3)}),
    "iql": (dict(value_head=True), dict(iql_expectile=0.7), {"iql_stats": (0, 2)}),
    "dist": (dict(spread_head=True), dict(distributional=True), {"dist_stats": (0, 2)}),
    "bcq": (dict(policy_head=True), dict(bcq_threshold=0.3), {"bcq_stats": (0, 3)}),
}


def _stepper(mode, dtype):
    from video_dqn_amd import synth
    from video_dqn_amd.engine import NetEngine, TDStepper
    net_kw, step_kw, _ = MODES[mode]
    net = NetEngine(3, 5, 1, True, dtype, 2 * B, deterministic=True, **net_kw)
    net.load_tensors(synth.make_state_dict(7))
    g = torch.Generator().manual_seed(8)
    for name in net.head_keys:
        v = net.view(name)
        v.copy_((0.05 * torch.randn(v.shape, generator=g)).to(v.device))
    net.mark_dirty()
    stp = TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, **step_kw)
    stp.loss_stats.fill_(5.0)
    return net, stp


@pytest.fixture(scope="module")
def batch():
    from video_dqn_amd import synth
    (tup, raw) = synth.make_batch(101, B, 1, structured=True, reward_p=0.3)
    g = torch.Generator().manual_seed(9)
    mc_return = (2.0 * torch.rand((B, 5), generator=g) - 0.5).cuda()  # on both sides of the targets
    return (torch.from_numpy(raw[0]).cuda(), torch.from_numpy(raw[1]).cuda(), 0, tup[2].cuda(), tup[3].float().cuda(), tup[4].float().cuda()), mc_return


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mode", list(MODES))
def test_loss_stats_slots_views_and_bit_identity(mode, dtype, batch):
    from video_dqn_amd.algos import LOSS_SLOTS
    args, mc_return = batch
    kw = dict(mc_return=mc_return) if mode == "calql" else {}
    views = MODES[mode][2]
    (net_a, a), (net_b, b) = _stepper(mode, dtype), _stepper(mode, dtype)
    assert a.loss_stats.shape == (LOSS_SLOTS,) and a.loss_stats.dtype == torch.float32
    for name in ("cql_penalty", "mc_stats", "iql_stats", "dist_stats", "bcq_stats"):  # every name stays, whatever the mode
        assert getattr(a, name).untyped_storage().data_ptr() == a.loss_stats.untyped_storage().data_ptr()
    for name, (lo, hi) in views.items():
        v = getattr(a, name)
        assert v.data_ptr() == a.loss_stats.data_ptr() + 4 * lo and v.numel() == hi - lo
    a.step(*args, **kw)
    torch.cuda.synchronize()
    owned = {i for lo, hi in views.values() for i in range(lo, hi)}
    stats = a.loss_stats.cpu()
    for i in range(LOSS_SLOTS):
        assert (stats[i].item() != 5.0) == (i in owned), (mode, i, stats)
    assert torch.isfinite(stats).all() and torch.isfinite(a.loss).all()
    b.step(*args, **kw)
    a.step(*args, **kw)
    b.step(*args, **kw)
    torch.cuda.synchronize()
    assert torch.equal(a.loss, b.loss) and torch.equal(a.loss_stats, b.loss_stats)
    assert torch.equal(a.grads, b.grads) and torch.equal(net_a.params, net_b.params)
    assert a.grads.abs().max().item() > 0
