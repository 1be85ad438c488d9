"""Implicit Q-learning, host side: the float64 autograd oracle (tests/iql_oracle.py) against its closed form, the distance of every
generated input from the expectile weight's kink, the IQL_EXPECTILE config key and check_iql, the value head in the engine's
parameter table (storage-only engines), the checkpoint split, and the C ABI's four new exports and their argument checks (no GPU:
every call fails before it reaches the device)."""
import ctypes as C
import types

import pytest
import torch

import iql_oracle


def _weights(B, seed=3):
    return torch.rand(B, generator=torch.Generator().manual_seed(seed)) * 0.9 + 0.1


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0.7, 0.5, 0.9])
@pytest.mark.parametrize("loss_kind", [0, 1], ids=["l2", "huber"])
def test_autograd_gradient_equals_closed_form_f64(loss_kind, tau):
    for B, ldq, C_, A in iql_oracle.OPERATOR_SHAPES:
        inp = iql_oracle.inputs(B, 11, ldq=ldq, n_cat=C_, n_act=A)
        inp[0] = inp[0] * 2.5 if ldq == 64 and B == 96 else inp[0]  # |d| beyond 1: both Huber branches
        disc = torch.rand(B, generator=torch.Generator().manual_seed(5)) * 0.5 + 0.4
        for kw in (dict(), dict(weight=_weights(B), use_valid=False), dict(clip_rect=0, gamma=0.5), dict(discount=disc)):
            kw = dict(kw, loss_kind=loss_kind, n_cat=C_, n_act=A)
            o = iql_oracle.objective(inp, tau, **kw)
            c = iql_oracle.closed_form(inp, tau, **kw)
            assert (o["dq"] - c).abs().max().item() <= 1e-12 * max(o["dq"].abs().max().item(), 1e-300)
            assert o["loss"].item() >= o["v_loss"].item() >= 0
            # columns other than the taken action's and the value head's carry no gradient
            n = C_ * A
            taken = torch.zeros(B, n, dtype=torch.bool)
            taken[torch.arange(B).repeat_interleave(C_), (torch.arange(C_).repeat(B) * A + inp[3].repeat_interleave(C_))] = True
            assert torch.all(o["dq"][:, :n][~taken] == 0)


def test_expectile_one_half_is_half_the_squared_error():
    inp = iql_oracle.inputs(96, 12)
    o = iql_oracle.objective(inp, 0.5, use_valid=False)
    inv = 1.0 / (5 * 96)
    assert abs(o["v_loss"].item() - float(torch.tensor(inv).float()) * (0.5 * o["u"] ** 2).sum().item()) <= 1e-12 * o["v_loss"].item()
    # and tau above one half weighs positive advantages more
    hi = iql_oracle.objective(inp, 0.9, use_valid=False)
    pos = (o["u"] > 0)
    assert hi["v_loss"].item() != o["v_loss"].item() and pos.any() and (~pos).any()


def test_every_gpu_input_keeps_its_distance_from_the_kink():
    """min |u| >= 1e-3 over EVERY (sample, category) term of every input the GPU tests generate, none excluded: the float32 kernel
    and the float64 oracle then take the same side of the expectile weight."""
    for B, ldq, C_, A, seed in iql_oracle.CASES:
        m = iql_oracle.min_abs_u(iql_oracle.inputs(B, seed, ldq=ldq, n_cat=C_, n_act=A), n_cat=C_, n_act=A)
        assert m >= iql_oracle.MIN_ABS_U, (B, ldq, C_, A, seed, m)


# ---- the config key ------------------------------------------------------------------------------------------------------------------
def test_config_has_iql_expectile_and_check_run_is_silent_when_off(tmp_path):
    from video_dqn_amd.config import get_cfg_defaults
    from video_dqn_amd.trainer import check_iql, check_run
    c = get_cfg_defaults()
    assert c.IQL_EXPECTILE == 0.0 and isinstance(c.IQL_EXPECTILE, float)
    check_iql(c)
    for key in ("TRAIN_ON_GROUND_TRUTH", "LINEAR", "VALUE_LEARNING", "ONE_ACTION"):  # off: nothing new is refused
        off = c.clone()
        off[key] = True
        check_iql(off)
    off = c.clone()
    off.CQL_ALPHA = 1.0
    check_iql(off)
    c.SYNTHETIC_DATA = True
    check_run(c)
    c.IQL_EXPECTILE = 0.7
    check_run(c)
    import video_dqn_amd.config as config_module
    assert "IQL_EXPECTILE" in config_module.__doc__


@pytest.mark.parametrize("bad,key", [(dict(IQL_EXPECTILE=0.3), "IQL_EXPECTILE"), (dict(IQL_EXPECTILE=1.0), "IQL_EXPECTILE"),
                                     (dict(IQL_EXPECTILE=-0.7), "IQL_EXPECTILE"), (dict(IQL_EXPECTILE=float("nan")), "IQL_EXPECTILE"),
                                     (dict(IQL_EXPECTILE=0.7, TRAIN_ON_GROUND_TRUTH=True), "TRAIN_ON_GROUND_TRUTH"),
                                     (dict(IQL_EXPECTILE=0.7, LINEAR=True), "LINEAR"),
                                     (dict(IQL_EXPECTILE=0.7, VALUE_LEARNING=True), "VALUE_LEARNING"),
                                     (dict(IQL_EXPECTILE=0.7, ONE_ACTION=True), "ONE_ACTION"),
                                     (dict(IQL_EXPECTILE=0.7, CQL_ALPHA=1.0), "CQL_ALPHA"),
                                     (dict(IQL_EXPECTILE=0.7, CQL_CALIBRATED=True), "CQL_CALIBRATED"),
                                     (dict(IQL_EXPECTILE=0.7, MC_RETURN_FLOOR=True), "MC_RETURN_FLOOR")])
def test_check_iql_raises_by_key_name(bad, key):
    from video_dqn_amd.config import get_cfg_defaults
    from video_dqn_amd.trainer import check_iql
    c = get_cfg_defaults()
    for k, v in bad.items():
        c[k] = v
    with pytest.raises(ValueError, match=key) as e:
        check_iql(c)
    assert "IQL_EXPECTILE" in str(e.value)
    if key in ("CQL_ALPHA", "CQL_CALIBRATED", "MC_RETURN_FLOOR"):
        assert "out of scope" in str(e.value)


def test_run_train_checks_iql_before_any_device_work(tmp_path):
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.trainer import run_train
    (tmp_path / "config.yml").write_text("SYNTHETIC_DATA: True\nIQL_EXPECTILE: 0.7\nLINEAR: True\n")
    with pytest.raises(ValueError, match="LINEAR"):
        run_train(ExperimentConfig(str(tmp_path), device="cpu", tensorboard=False), log=lambda *a: None)


# ---- the parameter table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra_capacity", [True, False], ids=["extra_capacity", "basic"])
def test_value_head_slots_sit_directly_behind_the_q_layer(extra_capacity):
    from video_dqn_amd.engine import NetEngine
    top, in_f = ("top.4", 256) if extra_capacity else ("top", 512)
    net = NetEngine(3, 5, 1, extra_capacity, "f32", 8, device="cpu", value_head=True)
    plain = NetEngine(3, 5, 1, extra_capacity, "f32", 8, device="cpu")
    assert net.value_head and not plain.value_head and net.lib.vdqn_net_value_head(net.handle) == 1 and net.lib.vdqn_net_value_head(plain.handle) == 0
    s = net.slots
    assert s["value.weight"].shape == (5, in_f) and s["value.bias"].shape == (5,)
    assert s[top + ".weight"].shape == (15, in_f) and s[top + ".bias"].shape == (15,)
    assert s["value.weight"].offset == s[top + ".weight"].offset + s[top + ".weight"].numel
    assert s["value.bias"].offset == s[top + ".bias"].offset + s[top + ".bias"].numel
    assert s["value.weight"].kind == s["value.bias"].kind == 0 and s["value.weight"].stage == s[top + ".weight"].stage
    ref_ids = [p.param_id for n, p in s.items() if p.kind in (0, 1) and not n.startswith("value.")]
    assert sorted(ref_ids) == list(range(len(ref_ids)))
    assert (s["value.weight"].param_id, s["value.bias"].param_id) == (len(ref_ids), len(ref_ids) + 1)
    grown = net.trainable_numel - plain.trainable_numel  # (every tensor's end is padded to 16 bytes: 15 -> 16 and 20 -> 20 floats of bias)
    assert "value.weight" not in plain.slots and 5 * in_f + 5 - 3 <= grown <= 5 * in_f + 5 + 3
    # every slot the two engines share has the reference's shape and id; the views of the value-head engine do not overlap
    for n, p in plain.slots.items():
        assert (s[n].shape, s[n].param_id, s[n].kind, s[n].stage) == (p.shape, p.param_id, p.kind, p.stage), n
    spans = sorted((p.offset, p.offset + p.numel) for p in s.values() if p.kind in (0, 1))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def test_value_head_zero_is_net_create():
    """vdqn_net_create_v(cfg, 0) builds vdqn_net_create's table (tests/test_engine_layout_cpu.py holds that one to the record)."""
    from video_dqn_amd import _lib
    lib = _lib.load()
    for ec in (1, 0):
        tables = []
        for create in (lambda cfg, h: lib.vdqn_net_create(C.byref(cfg), C.byref(h)), lambda cfg, h: lib.vdqn_net_create_v(C.byref(cfg), 0, C.byref(h))):
            cfg, h = _lib.NetConfig(3, 5, 1, ec, _lib.VDQN_BF16, 16, 0), C.c_void_p()
            assert create(cfg, h) == 0
            info, rows = _lib.ParamInfo(), []
            for i in range(lib.vdqn_net_num_params(h)):
                assert lib.vdqn_net_param_info(h, i, C.byref(info)) == 0
                rows.append((info.name, info.offset, info.numel, tuple(info.shape), info.kind, info.param_id, info.stage))
            rows.append((lib.vdqn_net_packed_bytes(h), lib.vdqn_net_acts_bytes(h, 8), lib.vdqn_net_bwd_bytes(h, 8), lib.vdqn_net_trainable_numel(h)))
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
def test_checkpoint_keeps_reference_keys_and_round_trips_the_value_head(tmp_path, g1, extra_capacity):
    from oracle import ref_cpu
    from video_dqn_amd.model import HabitatDQNMultiAction
    from video_dqn_amd.trainer import load_optimizer_state_dict, load_value_head_state, save_checkpoint
    model = HabitatDQNMultiAction(3, 5, extra_capacity=extra_capacity, panorama=False, dtype="f32", device="cpu", value_head=True)
    stub = _stub(model)
    path = tmp_path / "sample3.torch"
    save_checkpoint(str(path), 3, model, stub)
    snap = torch.load(path, map_location="cpu")
    assert set(snap) == {"sample_number", "model_state_dict", "optimizer_state_dict", "value_head"}
    ref = g1["ec1_pano0" if extra_capacity else "ec0_pano0"]
    assert list(snap["model_state_dict"]) == ref["keys"]
    assert [list(v.shape) for v in snap["model_state_dict"].values()] == ref["shapes"]
    # the reference's class (restated in oracle/ref_cpu.py) and torch's Adam over it load the two dicts as they are
    theirs = ref_cpu.HabitatDQNMultiAction(3, 5, extra_capacity=extra_capacity, panorama=False)
    theirs.load_state_dict(snap["model_state_dict"], strict=True)
    adam = torch.optim.Adam(theirs.parameters(), lr=1e-3)
    adam.load_state_dict(snap["optimizer_state_dict"])
    ids = sorted(snap["optimizer_state_dict"]["state"])
    n_ref = len(ref["params"])
    assert snap["optimizer_state_dict"]["param_groups"][0]["params"] == list(range(n_ref)) and max(ids) < n_ref
    top = "top.4" if extra_capacity else "top"
    assert torch.equal(dict(theirs.named_parameters())[top + ".weight"], model.engine.view(top + ".weight"))
    # the value head, bit for bit, into a fresh model and stepper stub
    vh = snap["value_head"]
    assert set(vh) == {"state_dict", "optimizer_state"} and set(vh["state_dict"]) == set(vh["optimizer_state"]) == {"value.weight", "value.bias"}
    assert set(vh["optimizer_state"]["value.weight"]) == {"step", "exp_avg", "exp_avg_sq"}
    fresh = HabitatDQNMultiAction(3, 5, extra_capacity=extra_capacity, panorama=False, dtype="f32", device="cpu", value_head=True)
    fresh_stub = _stub(fresh, step=0, seed=2)
    fresh.load_state_dict(snap["model_state_dict"])  # (no value.*: they keep their initialisation, until the next line)
    load_optimizer_state_dict(fresh_stub, snap["optimizer_state_dict"])
    load_value_head_state(fresh_stub, vh)
    assert fresh_stub.adam_step == 3
    nt = model.engine.trainable_numel
    assert torch.equal(fresh.engine.params[:nt], model.engine.params[:nt])
    assert torch.equal(fresh_stub.exp_avg, stub.exp_avg) and torch.equal(fresh_stub.exp_avg_sq, stub.exp_avg_sq)
    # a model without the head: the checkpoint it always wrote
    plain = HabitatDQNMultiAction(3, 5, extra_capacity=extra_capacity, panorama=False, dtype="f32", device="cpu")
    save_checkpoint(str(tmp_path / "plain.torch"), 3, plain, _stub(plain))
    p = torch.load(tmp_path / "plain.torch", map_location="cpu")
    assert set(p) == {"sample_number", "model_state_dict", "optimizer_state_dict"} and list(p["model_state_dict"]) == ref["keys"]


def test_warm_start_from_a_dqn_state_dict_keeps_the_initialised_value_head(capsys):
    from video_dqn_amd import engine, synth
    from video_dqn_amd.model import HabitatDQNMultiAction
    model = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype="f32", device="cpu", value_head=True)
    vw, vb = model.engine.view("value.weight").clone(), model.engine.view("value.bias").clone()
    assert vw.abs().max() > 0 and vw.abs().max() <= 1 / 16  # nn.Linear's U(-1/sqrt(256), 1/sqrt(256))
    sd = synth.make_state_dict(7)
    engine._SAID.clear()  # (it is said once per process: an earlier test may have met it)
    model.load_state_dict(sd)
    model.engine.load_tensors(sd)
    assert capsys.readouterr().out.count("the value head keeps its initialisation") == 1
    assert torch.equal(model.engine.view("value.weight"), vw) and torch.equal(model.engine.view("value.bias"), vb)
    assert torch.equal(model.engine.view("top.4.weight"), sd["top.4.weight"]) and torch.equal(model.engine.view("top.4.bias"), sd["top.4.bias"])
    assert list(model.state_dict())[-2:] == ["value.weight", "value.bias"] and len(model.state_dict()) == 252
    with pytest.raises(Exception):
        HabitatDQNMultiAction(1, 5, extra_capacity=True, panorama=False, dtype="f32", device="cpu", value_head=True)  # one action column


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_iql_symbols_at_abi_16():
    from video_dqn_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("vdqn_td_loss_iql", "vdqn_net_create_v", "vdqn_net_value_head", "vdqn_net_td_forward_iql"):
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


def test_td_loss_iql_refuses_bad_arguments():
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def call(tau=0.7, **kw):
        return lib.vdqn_td_loss_iql(C.byref(_td_args(buf, **kw)), p, p, p, tau, p, None)
    assert lib.vdqn_td_loss_iql(None, p, p, p, 0.7, p, None) != 0
    for kw in (dict(q_before=None), dict(q_after_online=None), dict(q_after_target=None), dict(act=None), dict(rew=None), dict(term=None),
               dict(loss=None), dict(use_valid=1, valid=None), dict(batch=0), dict(ldq=19), dict(dtype=_lib.VDQN_F32X3), dict(dtype=7),
               dict(loss_kind=2), dict(linear=1), dict(tau=0.0), dict(tau=0.49), dict(tau=1.0), dict(tau=float("nan"))):
        assert call(**kw) != 0, kw
        assert b"vdqn_td_loss_iql" in lib.vdqn_last_error(), kw
    assert call(linear=1) != 0 and b"linear" in lib.vdqn_last_error()
    assert call(tau=1.0) != 0 and b"expectile" in lib.vdqn_last_error()
    assert call(ldq=19) != 0 and b"ldq" in lib.vdqn_last_error()


def test_net_entries_refuse_bad_arguments():
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    h = C.c_void_p()
    for cfg, vh, word in ((_lib.NetConfig(1, 5, 1, 1, _lib.VDQN_F32, 8, 0), 1, b"action_dim"), (_lib.NetConfig(3, 17, 1, 1, _lib.VDQN_F32, 8, 0), 1, b"64"),
                          (_lib.NetConfig(3, 5, 1, 1, _lib.VDQN_F32, 8, 0), 2, b"value_head")):
        assert lib.vdqn_net_create_v(C.byref(cfg), vh, C.byref(h)) != 0
        assert b"vdqn_net_create_v" in lib.vdqn_last_error() and word in lib.vdqn_last_error()
    assert lib.vdqn_net_value_head(None) == 0
    nets = []
    for vh in (0, 1):
        cfg, h = _lib.NetConfig(3, 5, 1, 1, _lib.VDQN_F32, 8, 0), C.c_void_p()
        assert lib.vdqn_net_create_v(C.byref(cfg), vh, C.byref(h)) == 0
        nets.append(h)
    plain, valued = nets
    try:
        a = _lib.StepArgs()
        assert lib.vdqn_net_td_forward_iql(None, C.byref(a), 0.7, p, None) != 0 and b"vdqn_net_td_forward_iql: null arg" in lib.vdqn_last_error()
        assert lib.vdqn_net_td_forward_iql(plain, C.byref(a), 0.7, p, None) != 0 and b"vdqn_net_td_forward_iql: the net has no value head" in lib.vdqn_last_error()
        a.train_on_ground_truth = 1
        assert lib.vdqn_net_td_forward_iql(valued, C.byref(a), 0.7, p, None) != 0 and b"train_on_ground_truth" in lib.vdqn_last_error()
        a.train_on_ground_truth, a.linear = 0, 1
        assert lib.vdqn_net_td_forward_iql(valued, C.byref(a), 0.7, p, None) != 0 and b"vdqn_net_td_forward_iql: linear" in lib.vdqn_last_error()
        a.linear = 0
        for tau in (0.0, 0.3, 1.0, float("nan")):
            assert lib.vdqn_net_td_forward_iql(valued, C.byref(a), tau, p, None) != 0 and b"vdqn_net_td_forward_iql: expectile" in lib.vdqn_last_error()
        assert lib.vdqn_net_td_forward_iql(valued, C.byref(a), 0.7, p, None) != 0  # everything else missing: the shared entry's check
        assert b"null buffer" in lib.vdqn_last_error()
    finally:
        for h in nets:
            lib.vdqn_net_destroy(h)


def test_python_surface_is_off_by_default():
    import inspect
    from video_dqn_amd import ops
    from video_dqn_amd.engine import NetEngine, TDStepper
    from video_dqn_amd.model import HabitatDQNMultiAction
    assert inspect.signature(TDStepper.__init__).parameters["iql_expectile"].default == 0.0
    assert inspect.signature(NetEngine.__init__).parameters["value_head"].default is False
    assert inspect.signature(HabitatDQNMultiAction.__init__).parameters["value_head"].default is False
    assert callable(ops.td_loss_iql) and hasattr(HabitatDQNMultiAction, "state_values")
