"""Discrete BCQ, host side: the float64 autograd oracle (tests/bcq_oracle.py) against its closed form and against the Double-DQN
target of the TD oracle, the distance of every generated input from the threshold's boundary and the share of targets the constraint
changes, the BCQ_* config keys and check_bcq, the policy head in the engine's parameter table (storage-only engines), the checkpoint
split, and the C ABI's five new exports and their argument checks (no GPU: every call fails before it reaches the device)."""
import ctypes as C
import math
import types

import pytest
import torch

import bcq_oracle


def _weights(B, seed=3):
    return torch.rand(B, generator=torch.Generator().manual_seed(seed)) * 0.9 + 0.1


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", bcq_oracle.THRESHOLDS)
@pytest.mark.parametrize("loss_kind", [0, 1], ids=["l2", "huber"])
def test_autograd_gradient_equals_closed_form_f64(loss_kind, threshold):
    for B, ldq, C_, A in bcq_oracle.OPERATOR_SHAPES:
        inp = bcq_oracle.inputs(B, 11, ldq=ldq, n_cat=C_, n_act=A)
        inp[0] = inp[0] * 2.5 if ldq == 64 and B == 96 else inp[0]  # |d| beyond 1: both Huber branches
        disc = torch.rand(B, generator=torch.Generator().manual_seed(5)) * 0.5 + 0.4
        for kw in (dict(), dict(weight=_weights(B), use_valid=False), dict(clip_rect=0, gamma=0.5), dict(discount=disc),
                   dict(bc_weight=0.5, logit_reg=0.0)):
            kw = dict(kw, loss_kind=loss_kind, n_cat=C_, n_act=A)
            o = bcq_oracle.objective(inp, threshold, **kw)
            c = bcq_oracle.closed_form(inp, threshold, **kw)
            assert (o["dq"] - c).abs().max().item() <= 1e-12 * max(o["dq"].abs().max().item(), 1e-300)
            assert o["loss"].item() >= o["td_loss"].item() >= 0 and o["ce"].item() > 0
            assert 0 <= o["constrained_share"].item() <= 1 + 1e-6 and 0 <= o["accuracy"].item() <= 1 + 1e-6  # (inv is a float32)
            # columns other than the taken action's and the logits' carry no gradient; every logit column does
            n = C_ * A
            taken = torch.zeros(B, n, dtype=torch.bool)
            taken[torch.arange(B).repeat_interleave(C_), (torch.arange(C_).repeat(B) * A + inp[3].repeat_interleave(C_))] = True
            assert torch.all(o["dq"][:, :n][~taken] == 0) and torch.all(o["dq"][:, n:] != 0)
            if threshold == 0.0:
                assert o["constrained_share"].item() == 0.0


def test_threshold_zero_is_the_double_dqn_target_of_the_td_oracle():
    """With every action allowed the target, the TD error and the Q columns of the gradient are those of tests/cql_oracle.py at
    alpha = 0 (the oracle of vdqn_td_loss_weighted); with a threshold the best allowed action's target value is used."""
    import cql_oracle
    for B, ldq, C_, A in bcq_oracle.OPERATOR_SHAPES:
        inp = bcq_oracle.inputs(B, 12, ldq=ldq, n_cat=C_, n_act=A)
        w = _weights(B)
        for loss_kind in (0, 1):
            kw = dict(weight=w, use_valid=True, loss_kind=loss_kind, n_cat=C_, n_act=A, gamma=0.5)  # (a discount float32 holds exactly)
            o = bcq_oracle.objective(inp, 0.0, **kw)
            ref = cql_oracle.objective(inp, 0.0, **kw)
            n = C_ * A
            # (this oracle multiplies by the float32 inv_count the kernel is handed, that one by 1 / (C B) in float64: one part in 2^24)
            assert (o["dq"][:, :n] - ref["dq"][:, :n]).abs().max().item() <= 2.0 ** -23 * ref["dq"].abs().max().item()
            assert abs(o["td_loss"].item() - ref["loss"].item()) <= 2.0 ** -23 * abs(ref["loss"].item())
            assert (o["err"] - ref["err"]).abs().max().item() <= 1e-14
    # a threshold: y is taken at the best ALLOWED action
    inp = bcq_oracle.inputs(96, 12)
    o = bcq_oracle.objective(inp, 0.3, use_valid=False, clip_rect=0)
    ok = bcq_oracle.allowed_set(inp[1].double(), 0.3, 5, 3)
    assert ok.any(1).all() and not ok.all()
    assert ok.gather(1, o["best"]).all()  # every chosen action is allowed
    q3 = inp[1][:, :15].double().view(96, 5, 3)
    masked = torch.where(ok.view(96, 1, 3), q3, torch.full_like(q3, -math.inf))
    assert torch.equal(masked.max(2).values, q3.gather(2, o["best"].unsqueeze(2)).squeeze(2))


def test_every_gpu_input_keeps_its_margins_and_the_constraint_bites():
    """(a) margin >= 1e-3 on both counts for every threshold the GPU tests use, over every input they generate: the float32 kernel and
    the float64 oracle then take the same branch.  (b) threshold 0.3 changes between 10 % and 90 % of the (b, c) targets at every
    shape with B >= 3."""
    for B, ldq, C_, A, seed in bcq_oracle.CASES:
        inp = bcq_oracle.inputs(B, seed, ldq=ldq, n_cat=C_, n_act=A)
        for t in bcq_oracle.THRESHOLDS:
            m_logit, m_gap = bcq_oracle.margin(inp, t, n_cat=C_, n_act=A)
            assert m_logit >= bcq_oracle.MARGIN and m_gap >= bcq_oracle.MARGIN, (B, ldq, C_, A, seed, t, m_logit, m_gap)
        if B >= 3:
            share = bcq_oracle.changed_share(inp, 0.3, n_cat=C_, n_act=A)
            assert 0.1 <= share <= 0.9, (B, ldq, C_, A, seed, share)
        assert bcq_oracle.changed_share(inp, 0.0, n_cat=C_, n_act=A) == 0.0


# ---- the config keys -----------------------------------------------------------------------------------------------------------------
def test_config_has_the_bcq_keys_and_check_run_is_silent_when_off():
    from video_dqn_amd.config import get_cfg_defaults
    from video_dqn_amd.trainer import check_bcq, check_run
    c = get_cfg_defaults()
    assert (c.BCQ_THRESHOLD, c.BCQ_BC_WEIGHT, c.BCQ_LOGIT_REG) == (-1.0, 1.0, 0.01)
    assert all(isinstance(c[k], float) for k in ("BCQ_THRESHOLD", "BCQ_BC_WEIGHT", "BCQ_LOGIT_REG"))
    check_bcq(c)
    for key in ("TRAIN_ON_GROUND_TRUTH", "LINEAR", "VALUE_LEARNING", "ONE_ACTION", "CQL_CALIBRATED", "MC_RETURN_FLOOR", "DISTRIBUTIONAL"):
        off = c.clone()  # off: nothing new is refused
        off[key] = True
        check_bcq(off)
    off = c.clone()
    off.CQL_ALPHA, off.IQL_EXPECTILE = 1.0, 0.7
    check_bcq(off)
    c.SYNTHETIC_DATA = True
    check_run(c)
    for tau in (0.0, 0.3, 0.999):
        c.BCQ_THRESHOLD = tau
        check_run(c)
    c.N_STEP, c.LOSS_KIND, c.TARGET_TAU = 1, "huber", 0.01
    check_bcq(c)
    import video_dqn_amd.config as config_module
    for key in ("BCQ_THRESHOLD", "BCQ_BC_WEIGHT", "BCQ_LOGIT_REG"):
        assert key in config_module.__doc__


@pytest.mark.parametrize("bad,key", [(dict(BCQ_THRESHOLD=1.0), "BCQ_THRESHOLD"), (dict(BCQ_THRESHOLD=-0.5), "BCQ_THRESHOLD"),
                                     (dict(BCQ_THRESHOLD=-2.0), "BCQ_THRESHOLD"), (dict(BCQ_THRESHOLD=float("nan")), "BCQ_THRESHOLD"),
                                     (dict(BCQ_THRESHOLD=float("inf")), "BCQ_THRESHOLD"),
                                     (dict(BCQ_THRESHOLD=0.3, BCQ_BC_WEIGHT=0.0), "BCQ_BC_WEIGHT"),
                                     (dict(BCQ_THRESHOLD=0.3, BCQ_BC_WEIGHT=float("inf")), "BCQ_BC_WEIGHT"),
                                     (dict(BCQ_THRESHOLD=0.3, BCQ_LOGIT_REG=-0.1), "BCQ_LOGIT_REG"),
                                     (dict(BCQ_THRESHOLD=0.3, BCQ_LOGIT_REG=float("nan")), "BCQ_LOGIT_REG"),
                                     (dict(BCQ_BC_WEIGHT=2.0), "BCQ_BC_WEIGHT"), (dict(BCQ_LOGIT_REG=0.0), "BCQ_LOGIT_REG"),
                                     (dict(BCQ_THRESHOLD=0.3, TRAIN_ON_GROUND_TRUTH=True), "TRAIN_ON_GROUND_TRUTH"),
                                     (dict(BCQ_THRESHOLD=0.3, LINEAR=True), "LINEAR"),
                                     (dict(BCQ_THRESHOLD=0.3, VALUE_LEARNING=True), "VALUE_LEARNING"),
                                     (dict(BCQ_THRESHOLD=0.3, ONE_ACTION=True), "ONE_ACTION"),
                                     (dict(BCQ_THRESHOLD=0.3, CQL_ALPHA=1.0), "CQL_ALPHA"),
                                     (dict(BCQ_THRESHOLD=0.3, CQL_CALIBRATED=True), "CQL_CALIBRATED"),
                                     (dict(BCQ_THRESHOLD=0.3, MC_RETURN_FLOOR=True), "MC_RETURN_FLOOR"),
                                     (dict(BCQ_THRESHOLD=0.0, IQL_EXPECTILE=0.7), "IQL_EXPECTILE"),
                                     (dict(BCQ_THRESHOLD=0.3, DISTRIBUTIONAL=True), "DISTRIBUTIONAL")])
def test_check_bcq_raises_by_key_name(bad, key):
    from video_dqn_amd.config import get_cfg_defaults
    from video_dqn_amd.trainer import check_bcq
    c = get_cfg_defaults()
    for k, v in bad.items():
        c[k] = v
    with pytest.raises(ValueError, match=key) as e:
        check_bcq(c)
    assert "BCQ_" in str(e.value)
    if key in ("CQL_ALPHA", "CQL_CALIBRATED", "MC_RETURN_FLOOR", "IQL_EXPECTILE", "DISTRIBUTIONAL"):
        assert "out of scope" in str(e.value) and "BCQ_THRESHOLD" in str(e.value)
    if set(bad) in ({"BCQ_BC_WEIGHT"}, {"BCQ_LOGIT_REG"}):
        assert "no effect" in str(e.value)


def test_run_train_checks_bcq_before_any_device_work(tmp_path):
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.trainer import run_train
    (tmp_path / "config.yml").write_text("SYNTHETIC_DATA: True\nBCQ_THRESHOLD: 0.3\nLINEAR: True\n")
    with pytest.raises(ValueError, match="LINEAR"):
        run_train(ExperimentConfig(str(tmp_path), device="cpu", tensorboard=False), log=lambda *a: None)
    (tmp_path / "config.yml").write_text("SYNTHETIC_DATA: True\nBCQ_THRESHOLD: 1.5\n")
    with pytest.raises(ValueError, match="BCQ_THRESHOLD"):
        run_train(ExperimentConfig(str(tmp_path), device="cpu", tensorboard=False), log=lambda *a: None)


# ---- the parameter table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra_capacity", [True, False], ids=["extra_capacity", "basic"])
def test_policy_head_slots_sit_directly_behind_the_q_layer(extra_capacity):
    from video_dqn_amd.engine import NetEngine
    top, in_f = ("top.4", 256) if extra_capacity else ("top", 512)
    net = NetEngine(3, 5, 1, extra_capacity, "f32", 8, device="cpu", policy_head=True)
    plain = NetEngine(3, 5, 1, extra_capacity, "f32", 8, device="cpu")
    assert net.policy_head and not plain.policy_head and net.lib.vdqn_net_policy_head(net.handle) == 1 and net.lib.vdqn_net_policy_head(plain.handle) == 0
    assert net.lib.vdqn_net_value_head(net.handle) == 0 and net.lib.vdqn_net_spread_head(net.handle) == 0
    assert net.head == "policy" and net.head_keys == ("policy.weight", "policy.bias")
    s = net.slots
    assert s["policy.weight"].shape == (3, in_f) and s["policy.bias"].shape == (3,)
    assert s[top + ".weight"].shape == (15, in_f) and s[top + ".bias"].shape == (15,)
    assert s["policy.weight"].offset == s[top + ".weight"].offset + s[top + ".weight"].numel
    assert s["policy.bias"].offset == s[top + ".bias"].offset + s[top + ".bias"].numel
    assert s["policy.weight"].kind == s["policy.bias"].kind == 0 and s["policy.weight"].stage == s[top + ".weight"].stage
    ref_ids = [p.param_id for n, p in s.items() if p.kind in (0, 1) and not n.startswith("policy.")]
    assert sorted(ref_ids) == list(range(len(ref_ids)))
    assert (s["policy.weight"].param_id, s["policy.bias"].param_id) == (len(ref_ids), len(ref_ids) + 1)
    grown = net.trainable_numel - plain.trainable_numel  # (every tensor's end is padded to 16 bytes)
    assert "policy.weight" not in plain.slots and 3 * in_f + 3 - 3 <= grown <= 3 * in_f + 3 + 3
    for n, p in plain.slots.items():
        assert (s[n].shape, s[n].param_id, s[n].kind, s[n].stage) == (p.shape, p.param_id, p.kind, p.stage), n
    spans = sorted((p.offset, p.offset + p.numel) for p in s.values() if p.kind in (0, 1))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def test_policy_head_zero_is_net_create_d():
    """vdqn_net_create_p(cfg, v, s, 0) builds vdqn_net_create_d(cfg, v, s)'s table, for no head, the value head and the spread head."""
    from video_dqn_amd import _lib
    lib = _lib.load()
    for ec in (1, 0):
        for vh, sh in ((0, 0), (1, 0), (0, 1)):
            tables = []
            for create in (lambda cfg, h: lib.vdqn_net_create_d(C.byref(cfg), vh, sh, C.byref(h)),
                           lambda cfg, h: lib.vdqn_net_create_p(C.byref(cfg), vh, sh, 0, C.byref(h))):
                cfg, h = _lib.NetConfig(3, 5, 1, ec, _lib.VDQN_BF16, 16, 0), C.c_void_p()
                assert create(cfg, h) == 0
                info, rows = _lib.ParamInfo(), []
                for i in range(lib.vdqn_net_num_params(h)):
                    assert lib.vdqn_net_param_info(h, i, C.byref(info)) == 0
                    rows.append((info.name, info.offset, info.numel, tuple(info.shape), info.kind, info.param_id, info.stage))
                rows.append((lib.vdqn_net_packed_bytes(h), lib.vdqn_net_acts_bytes(h, 8), lib.vdqn_net_bwd_bytes(h, 8), lib.vdqn_net_trainable_numel(h)))
                assert lib.vdqn_net_policy_head(h) == 0
                tables.append(rows)
                lib.vdqn_net_destroy(h)
            assert tables[0] == tables[1]


# ---- the checkpoint -------------------------------------------------------------------------------------------------------------------
def _stub(model, step=3, seed=1):
    net = model.engine
    g = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(net=net, adam_step=step, exp_avg=torch.randn(net.trainable_numel, generator=g),
                                 exp_avg_sq=torch.rand(net.trainable_numel, generator=g), lr=1e-4, betas=(0.9, 0.999), eps=1e-8,
                                 weight_decay=0.0, lr_fn=None)


@pytest.mark.parametrize("extra_capacity", [True, False], ids=["extra_capacity", "basic"])
def test_checkpoint_keeps_reference_keys_and_round_trips_the_policy_head(tmp_path, g1, extra_capacity):
    from oracle import ref_cpu
    from video_dqn_amd.model import HabitatDQNMultiAction
    from video_dqn_amd.trainer import load_head_state, load_optimizer_state_dict, save_checkpoint
    model = HabitatDQNMultiAction(3, 5, extra_capacity=extra_capacity, panorama=False, dtype="f32", device="cpu", policy_head=True)
    stub = _stub(model)
    path = tmp_path / "sample3.torch"
    save_checkpoint(str(path), 3, model, stub)
    snap = torch.load(path, map_location="cpu")
    assert set(snap) == {"sample_number", "model_state_dict", "optimizer_state_dict", "policy_head"}
    ref = g1["ec1_pano0" if extra_capacity else "ec0_pano0"]
    assert list(snap["model_state_dict"]) == ref["keys"]
    assert [list(v.shape) for v in snap["model_state_dict"].values()] == ref["shapes"]
    theirs = ref_cpu.HabitatDQNMultiAction(3, 5, extra_capacity=extra_capacity, panorama=False)
    theirs.load_state_dict(snap["model_state_dict"], strict=True)
    adam = torch.optim.Adam(theirs.parameters(), lr=1e-3)
    adam.load_state_dict(snap["optimizer_state_dict"])
    ids = sorted(snap["optimizer_state_dict"]["state"])
    n_ref = len(ref["params"])
    assert snap["optimizer_state_dict"]["param_groups"][0]["params"] == list(range(n_ref)) and max(ids) < n_ref
    top = "top.4" if extra_capacity else "top"
    assert torch.equal(dict(theirs.named_parameters())[top + ".weight"], model.engine.view(top + ".weight"))
    ph = snap["policy_head"]
    assert set(ph) == {"state_dict", "optimizer_state"} and set(ph["state_dict"]) == set(ph["optimizer_state"]) == {"policy.weight", "policy.bias"}
    assert set(ph["optimizer_state"]["policy.weight"]) == {"step", "exp_avg", "exp_avg_sq"}
    # under TARGET_TAU the target's copy of the head is never read (the loss takes the ONLINE logits): it does not travel, as value_head's
    save_checkpoint(str(tmp_path / "soft.torch"), 3, model, stub, target_state_dict=snap["model_state_dict"])
    assert set(torch.load(tmp_path / "soft.torch", map_location="cpu")["policy_head"]) == {"state_dict", "optimizer_state"}
    fresh = HabitatDQNMultiAction(3, 5, extra_capacity=extra_capacity, panorama=False, dtype="f32", device="cpu", policy_head=True)
    fresh_stub = _stub(fresh, step=0, seed=2)
    fresh.load_state_dict(snap["model_state_dict"])  # (no policy.*: they keep their initialisation, until the next lines)
    load_optimizer_state_dict(fresh_stub, snap["optimizer_state_dict"])
    load_head_state(fresh_stub, ph)
    assert fresh_stub.adam_step == 3
    nt = model.engine.trainable_numel
    assert torch.equal(fresh.engine.params[:nt], model.engine.params[:nt])
    for sl in (slice(p.offset, p.offset + p.numel) for p in model.engine.slots.values() if p.kind == 0):  # (not the padding between tensors)
        assert torch.equal(fresh_stub.exp_avg[sl], stub.exp_avg[sl]) and torch.equal(fresh_stub.exp_avg_sq[sl], stub.exp_avg_sq[sl])
    plain = HabitatDQNMultiAction(3, 5, extra_capacity=extra_capacity, panorama=False, dtype="f32", device="cpu")
    save_checkpoint(str(tmp_path / "plain.torch"), 3, plain, _stub(plain))
    p = torch.load(tmp_path / "plain.torch", map_location="cpu")
    assert set(p) == {"sample_number", "model_state_dict", "optimizer_state_dict"} and list(p["model_state_dict"]) == ref["keys"]


def test_warm_start_from_a_dqn_state_dict_keeps_the_initialised_policy_head(capsys):
    from video_dqn_amd import engine, synth
    from video_dqn_amd.model import HabitatDQNMultiAction
    model = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype="f32", device="cpu", policy_head=True)
    pw, pb = model.engine.view("policy.weight").clone(), model.engine.view("policy.bias").clone()
    assert pw.abs().max() > 0 and pw.abs().max() <= 1 / 16  # nn.Linear's U(-1/sqrt(256), 1/sqrt(256))
    sd = synth.make_state_dict(7)
    engine._SAID.clear()  # (it is said once per process: an earlier test may have met it)
    model.load_state_dict(sd)
    model.engine.load_tensors(sd)
    assert capsys.readouterr().out.count("the policy head keeps its initialisation") == 1
    assert torch.equal(model.engine.view("policy.weight"), pw) and torch.equal(model.engine.view("policy.bias"), pb)
    assert torch.equal(model.engine.view("top.4.weight"), sd["top.4.weight"]) and torch.equal(model.engine.view("top.4.bias"), sd["top.4.bias"])
    assert list(model.state_dict())[-2:] == ["policy.weight", "policy.bias"] and len(model.state_dict()) == 252
    with pytest.raises(Exception):
        HabitatDQNMultiAction(1, 5, extra_capacity=True, panorama=False, dtype="f32", device="cpu", policy_head=True)  # one action column


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_bcq_symbols_at_abi_16():
    from video_dqn_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("vdqn_td_loss_bcq", "vdqn_bcq_constrain", "vdqn_net_create_p", "vdqn_net_policy_head", "vdqn_net_td_forward_bcq"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    loaded = _lib.load()
    assert loaded.vdqn_abi_version() == 16 == _lib.ABI_VERSION
    assert loaded.vdqn_abi_struct_size(7) == -1  # no new argument struct


def _td_args(buf, **kw):
    from video_dqn_amd import _lib
    a = _lib.TdArgs()
    p = C.addressof(buf)  # host memory, never dereferenced: every call below fails its argument check
    a.q_before = a.q_after_online = a.q_after_target = a.act = a.rew = a.term = a.valid = a.loss = a.dq = p
    a.batch, a.n_cat, a.n_act, a.ldq = 4, 5, 3, 64
    a.gamma, a.inv_count, a.clip_rect, a.dtype = 0.9, 0.05, 1, _lib.VDQN_F32
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_td_loss_bcq_refuses_bad_arguments():
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def call(threshold=0.3, bc_weight=1.0, logit_reg=0.01, **kw):
        return lib.vdqn_td_loss_bcq(C.byref(_td_args(buf, **kw)), p, p, p, threshold, bc_weight, logit_reg, p, None)
    assert lib.vdqn_td_loss_bcq(None, p, p, p, 0.3, 1.0, 0.01, p, None) != 0
    nan, inf = float("nan"), float("inf")
    for kw in (dict(q_before=None), dict(q_after_online=None), dict(q_after_target=None), dict(act=None), dict(rew=None), dict(term=None),
               dict(loss=None), dict(use_valid=1, valid=None), dict(batch=0), dict(n_cat=0), dict(ldq=17), dict(batch=1 << 25, ldq=64),
               dict(dtype=_lib.VDQN_F32X3), dict(dtype=7), dict(loss_kind=2), dict(loss_kind=-1), dict(linear=1), dict(n_act=1),
               dict(threshold=1.0), dict(threshold=-0.1), dict(threshold=-1.0), dict(threshold=nan), dict(threshold=inf),
               dict(bc_weight=0.0), dict(bc_weight=-1.0), dict(bc_weight=inf), dict(bc_weight=nan),
               dict(logit_reg=-0.01), dict(logit_reg=inf), dict(logit_reg=nan)):
        assert call(**kw) != 0, kw
        assert b"vdqn_td_loss_bcq" in lib.vdqn_last_error(), kw
    assert call(linear=1) != 0 and b"linear" in lib.vdqn_last_error()
    assert call(threshold=1.0) != 0 and b"threshold" in lib.vdqn_last_error()
    assert call(ldq=17) != 0 and b"ldq" in lib.vdqn_last_error()
    assert call(n_act=1) != 0 and b"n_act" in lib.vdqn_last_error()
    assert call(bc_weight=0.0) != 0 and b"bc_weight" in lib.vdqn_last_error()
    assert call(logit_reg=-0.01) != 0 and b"logit_reg" in lib.vdqn_last_error()
    assert call(batch=1 << 25) != 0 and b"32-bit" in lib.vdqn_last_error()


def test_bcq_constrain_refuses_bad_arguments():
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    good = dict(q=p, out=p, prob=None, batch=4, n_cat=5, n_act=3, ldq=64, threshold=0.3)
    for kw in (dict(q=None), dict(out=None), dict(batch=0), dict(n_cat=0), dict(n_act=1), dict(ldq=17), dict(batch=1 << 25),
               dict(threshold=1.0), dict(threshold=-1.0), dict(threshold=float("nan"))):
        k = dict(good, **kw)
        assert lib.vdqn_bcq_constrain(k["q"], k["out"], k["prob"], k["batch"], k["n_cat"], k["n_act"], k["ldq"], k["threshold"], None) != 0, kw
        assert b"vdqn_bcq_constrain" in lib.vdqn_last_error(), kw


def test_net_entries_refuse_bad_arguments():
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    h = C.c_void_p()
    ok = lambda: _lib.NetConfig(3, 5, 1, 1, _lib.VDQN_F32, 8, 0)  # noqa: E731
    for cfg, vh, sh, ph, word in ((_lib.NetConfig(1, 5, 1, 1, _lib.VDQN_F32, 8, 0), 0, 0, 1, b"action_dim"),
                                  (_lib.NetConfig(3, 21, 1, 1, _lib.VDQN_F32, 8, 0), 0, 0, 1, b"64"),
                                  (ok(), 0, 0, 2, b"policy_head"), (ok(), 0, 0, -1, b"policy_head"),
                                  (ok(), 1, 0, 1, b"out of scope"), (ok(), 0, 1, 1, b"out of scope"), (ok(), 2, 0, 1, b"value_head")):
        assert lib.vdqn_net_create_p(C.byref(cfg), vh, sh, ph, C.byref(h)) != 0
        assert b"vdqn_net_create_p" in lib.vdqn_last_error() and word in lib.vdqn_last_error(), lib.vdqn_last_error()
    cfg = _lib.NetConfig(3, 20, 1, 1, _lib.VDQN_F32, 8, 0)  # 60 + 3 columns: fits
    assert lib.vdqn_net_create_p(C.byref(cfg), 0, 0, 1, C.byref(h)) == 0
    lib.vdqn_net_destroy(h)
    assert lib.vdqn_net_policy_head(None) == 0
    nets = []
    for ph in (0, 1):
        cfg, h = ok(), C.c_void_p()
        assert lib.vdqn_net_create_p(C.byref(cfg), 0, 0, ph, C.byref(h)) == 0
        nets.append(h)
    plain, headed = nets
    try:
        a = _lib.StepArgs()
        call = lambda net, t=0.3, w=1.0, r=0.01: lib.vdqn_net_td_forward_bcq(net, C.byref(a), t, w, r, p, None)  # noqa: E731
        assert call(None) != 0 and b"vdqn_net_td_forward_bcq: null arg" in lib.vdqn_last_error()
        assert call(plain) != 0 and b"vdqn_net_td_forward_bcq: the net has no policy head" in lib.vdqn_last_error()
        a.train_on_ground_truth = 1
        assert call(headed) != 0 and b"train_on_ground_truth" in lib.vdqn_last_error()
        a.train_on_ground_truth, a.linear = 0, 1
        assert call(headed) != 0 and b"vdqn_net_td_forward_bcq: linear" in lib.vdqn_last_error()
        a.linear = 0
        for t in (-1.0, 1.0, float("nan")):
            assert call(headed, t=t) != 0 and b"vdqn_net_td_forward_bcq: threshold" in lib.vdqn_last_error()
        for w in (0.0, float("inf")):
            assert call(headed, w=w) != 0 and b"vdqn_net_td_forward_bcq: bc_weight" in lib.vdqn_last_error()
        for r in (-1.0, float("nan")):
            assert call(headed, r=r) != 0 and b"vdqn_net_td_forward_bcq: logit_reg" in lib.vdqn_last_error()
        assert call(headed) != 0  # everything else missing: the shared entry's check
        assert b"null buffer" in lib.vdqn_last_error()
    finally:
        for h in nets:
            lib.vdqn_net_destroy(h)


def test_python_surface_is_off_by_default():
    import inspect
    from video_dqn_amd import ops
    from video_dqn_amd.engine import NetEngine, TDStepper
    from video_dqn_amd.model import HabitatDQNMultiAction
    sig = inspect.signature(TDStepper.__init__).parameters
    assert (sig["bcq_threshold"].default, sig["bcq_bc_weight"].default, sig["bcq_logit_reg"].default) == (-1.0, 1.0, 0.01)
    assert inspect.signature(NetEngine.__init__).parameters["policy_head"].default is False
    assert inspect.signature(HabitatDQNMultiAction.__init__).parameters["policy_head"].default is False
    assert callable(ops.td_loss_bcq) and callable(ops.bcq_constrain)
    assert hasattr(HabitatDQNMultiAction, "constrained_q") and hasattr(HabitatDQNMultiAction, "behaviour")
    plain = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype="f32", device="cpu")
    assert not plain.policy_head and plain.engine.head is None and len(plain.state_dict()) == 250
    with pytest.raises(RuntimeError, match="policy_head"):
        plain.behaviour(torch.zeros(1, 3, 224, 224))
