"""Gaussian distributional Q-learning, host side: the float64 oracle over torch's kl_divergence (tests/dist_oracle.py) against its
closed form, the arg-max and clamp margins of every generated input, the measured distance of the float32 restatement from the
oracle, the DISTRIBUTIONAL / KL_BACKWARDS / LOG_SIGMA / DIST_SIGMA_MIN keys and check_dist, the spread head in the engine's parameter
table (storage-only engines), the checkpoint split, and the C ABI's five new exports and their argument checks (no GPU: every call
fails before it reaches the device)."""
import ctypes as C
import types

import pytest
import torch

import dist_oracle


def _weights(B, seed=3):
    return torch.rand(B, generator=torch.Generator().manual_seed(seed)) * 0.9 + 0.1


def _discount(B, seed=6):
    return torch.rand(B, generator=torch.Generator().manual_seed(seed)) * 0.5 + 0.45


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kl_backwards,log_sigma", dist_oracle.FLAGS, ids=["fwd-softplus", "bwd-softplus", "fwd-logsigma", "bwd-logsigma"])
def test_autograd_over_torch_kl_equals_closed_form_f64(kl_backwards, log_sigma):
    """1e-12 of the largest element for dq, 1e-12 relative (absolute below 1) for every term's L; columns other than the two live
    ones per category carry no gradient; every term's L >= 0."""
    for B, ldq, C_, A in dist_oracle.OPERATOR_SHAPES:
        inp = dist_oracle.inputs(B, 11, ldq=ldq, n_cat=C_, n_act=A)
        for kw in (dict(), dict(weight=_weights(B), use_valid=False), dict(clip_rect=0, gamma=0.5), dict(discount=_discount(B)), dict(sigma_min=0.01)):
            kw = dict(kw, kl_backwards=kl_backwards, log_sigma=log_sigma, n_cat=C_, n_act=A)
            o = dist_oracle.objective(inp, **kw)
            dq, L = dist_oracle.closed_form(inp, **kw)
            assert (o["dq"] - dq).abs().max().item() <= 1e-12 * max(o["dq"].abs().max().item(), 1e-300)
            assert ((o["L"] - L).abs() / o["L"].abs().clamp(min=1)).max().item() <= 1e-12
            assert o["L"].min().item() >= 0 and o["v"].min().item() >= dist_oracle.smin2_of(kw.get("sigma_min", 0.1))
            n = C_ * A
            live = torch.zeros(B, 2 * n, dtype=torch.bool)
            rows, cols = torch.arange(B).repeat_interleave(C_), torch.arange(C_).repeat(B) * A + inp[3].repeat_interleave(C_)
            live[rows, cols] = True
            live[rows, n + cols] = True
            assert torch.all(o["dq"][~live] == 0)
            term = inp[5].bool()
            assert torch.all(o["v"][term] == dist_oracle.smin2_of(kw.get("sigma_min", 0.1)))  # g = 0: the floor


def test_clamped_rows_carry_no_rho_gradient_in_the_oracle():
    B, ldq, C_, A, seed = dist_oracle.TAILS_CASE
    inp = dist_oracle.inputs(B, seed)
    n = C_ * A
    for b, rho in enumerate((-9.0, 5.0, 30.0)):
        inp[0][b, n:2 * n] = rho
    for kb in (False, True):
        o = dist_oracle.objective(inp, kl_backwards=kb, log_sigma=True)
        dq, _ = dist_oracle.closed_form(inp, kl_backwards=kb, log_sigma=True)
        assert torch.all(o["dq"][:3, n:] == 0) and torch.all(dq[:3, n:] == 0) and torch.isfinite(o["dq"]).all()
        assert (o["dq"][3:, n:] != 0).any()


def test_every_gpu_input_keeps_its_argmax_and_clamp_margins():
    for B, ldq, C_, A, seed in dist_oracle.CASES:
        inp = dist_oracle.inputs(B, seed, ldq=ldq, n_cat=C_, n_act=A)
        gap, margin = dist_oracle.argmax_gap(inp, C_, A), dist_oracle.clamp_margin(inp, C_, A)
        assert gap >= dist_oracle.ARGMAX_GAP and margin >= dist_oracle.CLAMP_MARGIN, (B, ldq, C_, A, seed, gap, margin)


def test_restate_f32_is_within_1e_6_of_the_oracle():
    """The float32 restatement in the kernel's expression order against the float64 oracle over CASES, both flags, sigma_min 0.1 and
    0.01, weighted with a per-sample discount and not: the worst dq deviation in units of the largest dq element and the worst
    relative loss deviation (DESIGN.md 3q records both).  More than 1e-6 would mean an ill-conditioned expression order."""
    worst_dq = worst_loss = 0.0
    for B, ldq, C_, A, seed in dist_oracle.CASES:
        inp = dist_oracle.inputs(B, seed, ldq=ldq, n_cat=C_, n_act=A)
        for kb, ls in dist_oracle.FLAGS:
            for smin in (0.1, 0.01):
                for kw in (dict(), dict(weight=_weights(B), discount=_discount(B), use_valid=False)):
                    e_dq, e_loss = dist_oracle.deviation(inp, kl_backwards=kb, log_sigma=ls, sigma_min=smin, n_cat=C_, n_act=A, **kw)
                    worst_dq, worst_loss = max(worst_dq, e_dq), max(worst_loss, e_loss)
    print(f"restate_f32 against the float64 oracle: dq {worst_dq:.2e} of the largest element, loss {worst_loss:.2e} relative")
    assert worst_dq <= 1e-6 and worst_loss <= 1e-6


# ---- the config keys -----------------------------------------------------------------------------------------------------------------
def test_config_keys_and_check_run_is_silent_when_off():
    from video_dqn_amd.config import get_cfg_defaults
    from video_dqn_amd.trainer import check_dist, check_run
    c = get_cfg_defaults()
    assert c.DISTRIBUTIONAL is False and c.KL_BACKWARDS is False and c.LOG_SIGMA is False and c.DIST_SIGMA_MIN == 0.1
    check_dist(c)
    for key in ("TRAIN_ON_GROUND_TRUTH", "LINEAR", "MC_RETURN_FLOOR", "CQL_CALIBRATED"):  # off: nothing new is refused
        off = c.clone()
        off[key] = True
        check_dist(off)
    off = c.clone()
    off.CQL_ALPHA, off.IQL_EXPECTILE, off.LOSS_KIND = 1.0, 0.7, "huber"
    check_dist(off)
    c.SYNTHETIC_DATA = True
    check_run(c)
    for more in (dict(), dict(KL_BACKWARDS=True), dict(LOG_SIGMA=True), dict(ONE_ACTION=True), dict(TARGET_TAU=0.01), dict(DIST_SIGMA_MIN=1e-4),
                 dict(DIST_SIGMA_MIN=10.0), dict(ARCHITECTURE="basic")):
        on = c.clone()
        on.DISTRIBUTIONAL = True
        for k, v in more.items():
            on[k] = v
        check_run(on)
    import video_dqn_amd.config as config_module
    for key in ("DISTRIBUTIONAL", "KL_BACKWARDS", "LOG_SIGMA", "DIST_SIGMA_MIN"):
        assert key in config_module.__doc__


@pytest.mark.parametrize("bad,key", [(dict(DISTRIBUTIONAL=1), "DISTRIBUTIONAL"), (dict(DISTRIBUTIONAL="yes"), "DISTRIBUTIONAL"),
                                     (dict(DISTRIBUTIONAL=True, KL_BACKWARDS=1), "KL_BACKWARDS"), (dict(DISTRIBUTIONAL=True, LOG_SIGMA=0.5), "LOG_SIGMA"),
                                     (dict(KL_BACKWARDS=True), "KL_BACKWARDS"), (dict(LOG_SIGMA=True), "LOG_SIGMA"),
                                     (dict(DIST_SIGMA_MIN=0.0), "DIST_SIGMA_MIN"), (dict(DIST_SIGMA_MIN=5e-5), "DIST_SIGMA_MIN"),
                                     (dict(DIST_SIGMA_MIN=11.0), "DIST_SIGMA_MIN"), (dict(DIST_SIGMA_MIN=float("nan")), "DIST_SIGMA_MIN"),
                                     (dict(DIST_SIGMA_MIN=True), "DIST_SIGMA_MIN"),
                                     (dict(DISTRIBUTIONAL=True, TRAIN_ON_GROUND_TRUTH=True), "TRAIN_ON_GROUND_TRUTH"),
                                     (dict(DISTRIBUTIONAL=True, LINEAR=True), "LINEAR"),
                                     (dict(DISTRIBUTIONAL=True, LOSS_KIND="huber"), "LOSS_KIND"),
                                     (dict(DISTRIBUTIONAL=True, CQL_ALPHA=1.0), "CQL_ALPHA"),
                                     (dict(DISTRIBUTIONAL=True, CQL_CALIBRATED=True), "CQL_CALIBRATED"),
                                     (dict(DISTRIBUTIONAL=True, MC_RETURN_FLOOR=True), "MC_RETURN_FLOOR"),
                                     (dict(DISTRIBUTIONAL=True, IQL_EXPECTILE=0.7), "IQL_EXPECTILE")])
def test_check_dist_raises_by_key_name(bad, key):
    from video_dqn_amd.config import get_cfg_defaults
    from video_dqn_amd.trainer import check_dist
    c = types.SimpleNamespace(**dict(get_cfg_defaults()))  # (a plain record: the yacs node itself refuses a value of another type)
    for k, v in bad.items():
        setattr(c, k, v)
    with pytest.raises(ValueError, match=key) as e:
        check_dist(c)
    if key in ("KL_BACKWARDS", "LOG_SIGMA") and not bad.get("DISTRIBUTIONAL"):
        assert "has no effect" in str(e.value)
    if key in ("CQL_ALPHA", "CQL_CALIBRATED", "MC_RETURN_FLOOR", "IQL_EXPECTILE"):
        assert "out of scope" in str(e.value) and "DISTRIBUTIONAL" in str(e.value)


def test_run_train_checks_dist_before_any_device_work(tmp_path):
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.trainer import run_train
    for text, key in (("DISTRIBUTIONAL: True\nLINEAR: True\n", "LINEAR"), ("LOG_SIGMA: True\n", "LOG_SIGMA"),
                      ("DISTRIBUTIONAL: True\nLOSS_KIND: 'huber'\n", "LOSS_KIND")):
        (tmp_path / "config.yml").write_text("SYNTHETIC_DATA: True\n" + text)
        with pytest.raises(ValueError, match=key):
            run_train(ExperimentConfig(str(tmp_path), device="cpu", tensorboard=False), log=lambda *a: None)


# ---- the parameter table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra_capacity", [True, False], ids=["extra_capacity", "basic"])
def test_spread_head_slots_sit_directly_behind_the_q_layer(extra_capacity):
    from video_dqn_amd.engine import NetEngine
    top, in_f = ("top.4", 256) if extra_capacity else ("top", 512)
    net = NetEngine(3, 5, 1, extra_capacity, "f32", 8, device="cpu", spread_head=True)
    plain = NetEngine(3, 5, 1, extra_capacity, "f32", 8, device="cpu")
    assert net.spread_head and not plain.spread_head and not net.value_head
    assert net.lib.vdqn_net_spread_head(net.handle) == 1 and net.lib.vdqn_net_spread_head(plain.handle) == 0 and net.lib.vdqn_net_value_head(net.handle) == 0
    s = net.slots
    assert s["spread.weight"].shape == (15, in_f) and s["spread.bias"].shape == (15,)
    assert s[top + ".weight"].shape == (15, in_f) and s[top + ".bias"].shape == (15,)
    assert s["spread.weight"].offset == s[top + ".weight"].offset + s[top + ".weight"].numel
    assert s["spread.bias"].offset == s[top + ".bias"].offset + s[top + ".bias"].numel
    assert s["spread.weight"].kind == s["spread.bias"].kind == 0 and s["spread.weight"].stage == s[top + ".weight"].stage
    ref_ids = [p.param_id for n, p in s.items() if p.kind in (0, 1) and not n.startswith("spread.")]
    assert sorted(ref_ids) == list(range(len(ref_ids)))
    assert (s["spread.weight"].param_id, s["spread.bias"].param_id) == (len(ref_ids), len(ref_ids) + 1)
    assert "spread.weight" not in plain.slots and "value.weight" not in s
    for n, p in plain.slots.items():
        assert (s[n].shape, s[n].param_id, s[n].kind, s[n].stage) == (p.shape, p.param_id, p.kind, p.stage), n
    spans = sorted((p.offset, p.offset + p.numel) for p in s.values() if p.kind in (0, 1))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    one = NetEngine(1, 5, 1, extra_capacity, "f32", 8, device="cpu", spread_head=True)  # one action column is allowed
    assert one.slots["spread.weight"].shape == (5, in_f)


def test_spread_head_zero_is_net_create_v():
    """vdqn_net_create_d(cfg, v, 0) builds vdqn_net_create_v(cfg, v)'s table (tests/test_engine_layout_cpu.py holds v = 0 to the record)."""
    from video_dqn_amd import _lib
    lib = _lib.load()
    for ec in (1, 0):
        for vh in (0, 1):
            tables = []
            for create in (lambda cfg, h: lib.vdqn_net_create_v(C.byref(cfg), vh, C.byref(h)), lambda cfg, h: lib.vdqn_net_create_d(C.byref(cfg), vh, 0, C.byref(h))):
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
                                 weight_decay=0.0, lr_fn=None, target_params=torch.randn(net.params_numel, generator=g))


@pytest.mark.parametrize("extra_capacity", [True, False], ids=["extra_capacity", "basic"])
def test_checkpoint_keeps_reference_keys_and_round_trips_the_spread_head(tmp_path, extra_capacity):
    import json
    import os
    from oracle import ref_cpu
    from video_dqn_amd.model import HabitatDQNMultiAction
    from video_dqn_amd.trainer import head_state, load_head_state, load_optimizer_state_dict, save_checkpoint
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g1_state_dict.json")) as f:
        ref = json.load(f)["ec1_pano0" if extra_capacity else "ec0_pano0"]
    model = HabitatDQNMultiAction(3, 5, extra_capacity=extra_capacity, panorama=False, dtype="f32", device="cpu", distributional=True)
    stub = _stub(model)
    path = tmp_path / "sample3.torch"
    save_checkpoint(str(path), 3, model, stub)
    snap = torch.load(path, map_location="cpu")
    assert set(snap) == {"sample_number", "model_state_dict", "optimizer_state_dict", "spread_head"}
    assert list(snap["model_state_dict"]) == ref["keys"]
    assert [list(v.shape) for v in snap["model_state_dict"].values()] == ref["shapes"]
    theirs = ref_cpu.HabitatDQNMultiAction(3, 5, extra_capacity=extra_capacity, panorama=False)
    theirs.load_state_dict(snap["model_state_dict"], strict=True)
    adam = torch.optim.Adam(theirs.parameters(), lr=1e-3)
    adam.load_state_dict(snap["optimizer_state_dict"])
    n_ref = len(ref["params"])
    assert snap["optimizer_state_dict"]["param_groups"][0]["params"] == list(range(n_ref)) and max(snap["optimizer_state_dict"]["state"]) < n_ref
    sh = snap["spread_head"]
    assert set(sh) == {"state_dict", "optimizer_state"} and set(sh["state_dict"]) == set(sh["optimizer_state"]) == {"spread.weight", "spread.bias"}
    assert set(sh["optimizer_state"]["spread.weight"]) == {"step", "exp_avg", "exp_avg_sq"}
    fresh = HabitatDQNMultiAction(3, 5, extra_capacity=extra_capacity, panorama=False, dtype="f32", device="cpu", distributional=True)
    fresh_stub = _stub(fresh, step=0, seed=2)
    fresh.load_state_dict(snap["model_state_dict"])  # (no spread.*: they keep their initialisation, until the next lines)
    load_optimizer_state_dict(fresh_stub, snap["optimizer_state_dict"])
    load_head_state(fresh_stub, sh)
    assert fresh_stub.adam_step == 3
    nt = model.engine.trainable_numel
    assert torch.equal(fresh.engine.params[:nt], model.engine.params[:nt])
    for s in model.engine.slots.values():  # (slot by slot: the padding between two tensors belongs to nobody and is not stored)
        if s.kind == 0:
            sl = slice(s.offset, s.offset + s.numel)
            assert torch.equal(fresh_stub.exp_avg[sl], stub.exp_avg[sl]) and torch.equal(fresh_stub.exp_avg_sq[sl], stub.exp_avg_sq[sl]), s.name
    # TARGET_TAU: the target's spread rows travel in the head's own key, the reference-shaped target_state_dict stays as it was
    with_target = head_state(stub, with_target=True)
    s = model.engine.slots["spread.weight"]
    assert torch.equal(with_target["target_state_dict"]["spread.weight"], stub.target_params[s.offset:s.offset + s.numel].view(s.shape))
    save_checkpoint(str(tmp_path / "tau.torch"), 3, model, stub, target_state_dict={"stand-in": torch.zeros(1)})
    assert set(torch.load(tmp_path / "tau.torch", map_location="cpu")["spread_head"]) == {"state_dict", "optimizer_state", "target_state_dict"}
    # a model without the head: the checkpoint it always wrote
    plain = HabitatDQNMultiAction(3, 5, extra_capacity=extra_capacity, panorama=False, dtype="f32", device="cpu")
    save_checkpoint(str(tmp_path / "plain.torch"), 3, plain, _stub(plain))
    p = torch.load(tmp_path / "plain.torch", map_location="cpu")
    assert set(p) == {"sample_number", "model_state_dict", "optimizer_state_dict"} and list(p["model_state_dict"]) == ref["keys"]


def test_warm_start_from_a_dqn_state_dict_keeps_the_initialised_spread_head(capsys):
    from video_dqn_amd import engine, synth
    from video_dqn_amd.model import HabitatDQNMultiAction
    model = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype="f32", device="cpu", distributional=True)
    sw, sb = model.engine.view("spread.weight").clone(), model.engine.view("spread.bias").clone()
    assert sw.abs().max() > 0 and sw.abs().max() <= 1 / 16  # nn.Linear's U(-1/sqrt(256), 1/sqrt(256))
    sd = synth.make_state_dict(7)
    engine._SAID.clear()  # (it is said once per process: an earlier test may have met it)
    model.load_state_dict(sd)
    model.engine.load_tensors(sd)
    assert capsys.readouterr().out.count("the spread head keeps its initialisation") == 1
    assert torch.equal(model.engine.view("spread.weight"), sw) and torch.equal(model.engine.view("spread.bias"), sb)
    assert torch.equal(model.engine.view("top.4.weight"), sd["top.4.weight"]) and torch.equal(model.engine.view("top.4.bias"), sd["top.4.bias"])
    assert list(model.state_dict())[-2:] == ["spread.weight", "spread.bias"] and len(model.state_dict()) == 252
    assert isinstance(model.spread.weight, torch.nn.Parameter) and not hasattr(model, "value")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("vdqn_td_loss_dist", "vdqn_dist_moments", "vdqn_net_create_d", "vdqn_net_spread_head", "vdqn_net_td_forward_dist")


def test_library_exports_the_dist_symbols_at_abi_16():
    from video_dqn_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    loaded = _lib.load()
    assert loaded.vdqn_abi_version() == 16 == _lib.ABI_VERSION
    assert loaded.vdqn_abi_struct_size(7) == -1  # no new argument struct
    assert loaded.vdqn_abi_struct_size(6) == C.sizeof(_lib.StepArgs) and loaded.vdqn_abi_struct_size(2) == C.sizeof(_lib.TdArgs)  # as they were


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


def test_td_loss_dist_refuses_bad_arguments():
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def call(flags=0, smin=0.1, **kw):
        return lib.vdqn_td_loss_dist(C.byref(_td_args(buf, **kw)), p, p, p, flags, smin, p, None)
    assert lib.vdqn_td_loss_dist(None, p, p, p, 0, 0.1, p, None) != 0
    for kw in (dict(q_before=None), dict(q_after_online=None), dict(q_after_target=None), dict(act=None), dict(rew=None), dict(term=None),
               dict(loss=None), dict(use_valid=1, valid=None), dict(batch=0), dict(n_act=0), dict(ldq=29), dict(dtype=_lib.VDQN_F32X3), dict(dtype=7),
               dict(loss_kind=1), dict(linear=1), dict(flags=4), dict(flags=-1), dict(smin=0.0), dict(smin=5e-5), dict(smin=10.5),
               dict(smin=float("nan")), dict(smin=float("inf")), dict(batch=1 << 25, ldq=64)):
        assert call(**kw) != 0, kw
        assert b"vdqn_td_loss_dist" in lib.vdqn_last_error(), kw
    for kw, word in ((dict(linear=1), b"linear"), (dict(loss_kind=1), b"Huber"), (dict(ldq=29), b"ldq"), (dict(flags=8), b"unknown bits"),
                     (dict(smin=11.0), b"sigma_min"), (dict(batch=1 << 25, ldq=64), b"32-bit")):
        assert call(**kw) != 0 and word in lib.vdqn_last_error(), kw


def test_dist_moments_refuses_bad_arguments():
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    for args, word in (((None, p, 4, 5, 3, 64, 0, 0.1), b"null"), ((p, None, 4, 5, 3, 64, 0, 0.1), b"null"), ((p, p, 0, 5, 3, 64, 0, 0.1), b"bad dims"),
                       ((p, p, 4, 5, 3, 29, 0, 0.1), b"ldq"), ((p, p, 4, 5, 3, 64, 4, 0.1), b"unknown bits"), ((p, p, 4, 5, 3, 64, 2, 0.0), b"sigma_min"),
                       ((p, p, 1 << 25, 5, 3, 64, 0, 0.1), b"32-bit"), ((p, p + 4, 4, 5, 3, 64, 0, 0.1), b"aligned")):
        assert lib.vdqn_dist_moments(*args, None) != 0, args
        assert b"vdqn_dist_moments" in lib.vdqn_last_error() and word in lib.vdqn_last_error(), (args, lib.vdqn_last_error())


def test_net_entries_refuse_bad_arguments():
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    h = C.c_void_p()
    for cfg, vh, sh, word in ((_lib.NetConfig(3, 11, 1, 1, _lib.VDQN_F32, 8, 0), 0, 1, b"64"), (_lib.NetConfig(3, 5, 1, 1, _lib.VDQN_F32, 8, 0), 0, 2, b"spread_head"),
                              (_lib.NetConfig(3, 5, 1, 1, _lib.VDQN_F32, 8, 0), 1, 1, b"out of scope"), (_lib.NetConfig(3, 5, 1, 1, _lib.VDQN_F32, 8, 0), 2, 1, b"value_head")):
        assert lib.vdqn_net_create_d(C.byref(cfg), vh, sh, C.byref(h)) != 0
        assert b"vdqn_net_create_d" in lib.vdqn_last_error() and word in lib.vdqn_last_error(), lib.vdqn_last_error()
    assert lib.vdqn_net_spread_head(None) == 0
    nets = []
    for sh in (0, 1):
        cfg, h = _lib.NetConfig(3, 5, 1, 1, _lib.VDQN_F32, 8, 0), C.c_void_p()
        assert lib.vdqn_net_create_d(C.byref(cfg), 0, sh, C.byref(h)) == 0
        nets.append(h)
    plain, spread = nets
    try:
        a = _lib.StepArgs()
        name = b"vdqn_net_td_forward_dist: "
        assert lib.vdqn_net_td_forward_dist(None, C.byref(a), 0, 0.1, p, None) != 0 and name + b"null arg" in lib.vdqn_last_error()
        assert lib.vdqn_net_td_forward_dist(plain, C.byref(a), 0, 0.1, p, None) != 0 and name + b"the net has no spread head" in lib.vdqn_last_error()
        a.train_on_ground_truth = 1
        assert lib.vdqn_net_td_forward_dist(spread, C.byref(a), 0, 0.1, p, None) != 0 and b"train_on_ground_truth" in lib.vdqn_last_error()
        a.train_on_ground_truth, a.linear = 0, 1
        assert lib.vdqn_net_td_forward_dist(spread, C.byref(a), 0, 0.1, p, None) != 0 and name + b"linear" in lib.vdqn_last_error()
        a.linear, a.loss_kind = 0, 1
        assert lib.vdqn_net_td_forward_dist(spread, C.byref(a), 0, 0.1, p, None) != 0 and name + b"loss_kind" in lib.vdqn_last_error()
        a.loss_kind = 0
        assert lib.vdqn_net_td_forward_dist(spread, C.byref(a), 4, 0.1, p, None) != 0 and name + b"flags" in lib.vdqn_last_error()
        for smin in (0.0, 5e-5, 10.5, float("nan")):
            assert lib.vdqn_net_td_forward_dist(spread, C.byref(a), 3, smin, p, None) != 0 and name + b"sigma_min" in lib.vdqn_last_error()
        assert lib.vdqn_net_td_forward_dist(spread, C.byref(a), 3, 0.1, p, None) != 0  # everything else missing: the shared entry's check
        assert b"null buffer" in lib.vdqn_last_error()
        # the value-head entry refuses the spread-head net, and the other way round
        assert lib.vdqn_net_td_forward_iql(spread, C.byref(a), 0.7, p, None) != 0 and b"no value head" in lib.vdqn_last_error()
    finally:
        for h in nets:
            lib.vdqn_net_destroy(h)


def test_python_surface_is_off_by_default():
    import inspect
    from video_dqn_amd import ops
    from video_dqn_amd.engine import NetEngine, TDStepper
    from video_dqn_amd.model import HabitatDQNMultiAction
    sig = inspect.signature(TDStepper.__init__).parameters
    assert sig["distributional"].default is False and sig["kl_backwards"].default is False and sig["log_sigma"].default is False
    assert sig["sigma_min"].default == 0.1
    assert inspect.signature(NetEngine.__init__).parameters["spread_head"].default is False
    msig = inspect.signature(HabitatDQNMultiAction.__init__).parameters
    assert msig["distributional"].default is False and msig["log_sigma"].default is False and msig["sigma_min"].default == 0.1
    assert callable(ops.td_loss_dist) and callable(ops.dist_moments)
    plain = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype="f32", device="cpu")
    assert not plain.distributional and plain.engine.head is None and len(plain.state_dict()) == 250
    with pytest.raises(RuntimeError, match="distributional"):
        plain.distribution(torch.zeros(1, 3, 224, 224))
    with pytest.raises(Exception, match="out of scope"):
        NetEngine(3, 5, 1, True, "f32", 8, device="cpu", value_head=True, spread_head=True)
