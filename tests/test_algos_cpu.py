"""The table of head algorithms (video_dqn_amd/algos.py) against everything that reads it: the config checks over all on/off
combinations of the six loss keys, the engine's head tables, the statistics slots and the config keys.  No GPU."""
import ctypes as C
import itertools
import types

import pytest

KEYS_ON = (("CQL_ALPHA", 1.0), ("MC_RETURN_FLOOR", True), ("CQL_CALIBRATED", True), ("IQL_EXPECTILE", 0.7), ("DISTRIBUTIONAL", True),
           ("BCQ_THRESHOLD", 0.3))
TD_KEYS, HEAD_KEYS = ("CQL_ALPHA", "MC_RETURN_FLOOR", "CQL_CALIBRATED"), ("IQL_EXPECTILE", "DISTRIBUTIONAL", "BCQ_THRESHOLD")

# what check_cql, check_iql, check_dist, check_bcq accept between them: nothing, each head algorithm alone, and the TD family's keys
# in every combination (check_mc, which ties CQL_CALIBRATED to CQL_ALPHA, needs a dataset and is not part of this)
ACCEPTED = [(), ("IQL_EXPECTILE",), ("DISTRIBUTIONAL",), ("BCQ_THRESHOLD",), ("CQL_ALPHA",), ("MC_RETURN_FLOOR",), ("CQL_CALIBRATED",),
            ("CQL_ALPHA", "MC_RETURN_FLOOR"), ("CQL_ALPHA", "CQL_CALIBRATED"), ("MC_RETURN_FLOOR", "CQL_CALIBRATED"),
            ("CQL_ALPHA", "MC_RETURN_FLOOR", "CQL_CALIBRATED")]

NO_TABLE = "loss launch takes no Monte-Carlo return table; use one or the other"
ONE_HEAD = "is deliberately out of scope: one extra head sits behind the Q layer, the"
# the text of every refused pair, as the commit before the table raised it
PAIR_TEXT = {
    ("CQL_ALPHA", "IQL_EXPECTILE"): "IQL_EXPECTILE with CQL_ALPHA > 0 is deliberately out of scope: the IQL loss launch has no conservative penalty "
                                    "(implicit Q-learning avoids out-of-data actions instead of penalising them); use one or the other",
    ("CQL_ALPHA", "DISTRIBUTIONAL"): "DISTRIBUTIONAL with CQL_ALPHA > 0 is deliberately out of scope: the distributional loss launch has no "
                                     "conservative penalty; use one or the other",
    ("CQL_ALPHA", "BCQ_THRESHOLD"): "BCQ_THRESHOLD with CQL_ALPHA > 0 is deliberately out of scope: the BCQ loss launch has no conservative penalty; "
                                    "use one or the other",
    ("MC_RETURN_FLOOR", "IQL_EXPECTILE"): f"IQL_EXPECTILE with MC_RETURN_FLOOR is deliberately out of scope: the IQL {NO_TABLE}",
    ("MC_RETURN_FLOOR", "DISTRIBUTIONAL"): f"DISTRIBUTIONAL with MC_RETURN_FLOOR is deliberately out of scope: the distributional {NO_TABLE}",
    ("MC_RETURN_FLOOR", "BCQ_THRESHOLD"): f"BCQ_THRESHOLD with MC_RETURN_FLOOR is deliberately out of scope: the BCQ {NO_TABLE}",
    ("CQL_CALIBRATED", "IQL_EXPECTILE"): f"IQL_EXPECTILE with CQL_CALIBRATED is deliberately out of scope: the IQL {NO_TABLE}",
    ("CQL_CALIBRATED", "DISTRIBUTIONAL"): f"DISTRIBUTIONAL with CQL_CALIBRATED is deliberately out of scope: the distributional {NO_TABLE}",
    ("CQL_CALIBRATED", "BCQ_THRESHOLD"): f"BCQ_THRESHOLD with CQL_CALIBRATED is deliberately out of scope: the BCQ {NO_TABLE}",
    ("IQL_EXPECTILE", "DISTRIBUTIONAL"): f"DISTRIBUTIONAL with IQL_EXPECTILE > 0 {ONE_HEAD} value head or the spread head; use one or the other",
    ("IQL_EXPECTILE", "BCQ_THRESHOLD"): f"BCQ_THRESHOLD with IQL_EXPECTILE > 0 {ONE_HEAD} value head or the policy head; use one or the other",
    ("DISTRIBUTIONAL", "BCQ_THRESHOLD"): f"BCQ_THRESHOLD with DISTRIBUTIONAL {ONE_HEAD} spread head or the policy head; use one or the other",
}


def _config(keys):
    from video_dqn_amd.config import get_cfg_defaults
    c = types.SimpleNamespace(**dict(get_cfg_defaults()))
    for k in keys:
        setattr(c, k, dict(KEYS_ON)[k])
    return c


def _all_checks(c):
    from video_dqn_amd import trainer
    for check in (trainer.check_cql, trainer.check_iql, trainer.check_dist, trainer.check_bcq):
        check(c)


def test_the_64_combinations_of_the_loss_keys():
    accepted = []
    for mask in itertools.product((False, True), repeat=len(KEYS_ON)):
        keys = tuple(k for (k, _), m in zip(KEYS_ON, mask) if m)
        try:
            _all_checks(_config(keys))
            accepted.append(keys)
        except ValueError as e:
            assert "out of scope" in str(e), (keys, str(e))
            if len(keys) == 2:
                assert keys[0] in str(e) and keys[1] in str(e)
                assert str(e) == PAIR_TEXT[keys]
    assert sorted(accepted) == sorted(ACCEPTED)
    refused_pairs = [p for p in itertools.combinations([k for k, _ in KEYS_ON], 2) if p not in ACCEPTED]
    assert sorted(refused_pairs) == sorted(PAIR_TEXT)  # (twelve: every head algorithm with every TD key, and the three pairs of heads)


@pytest.mark.parametrize("name,key", [("check_iql", "IQL_EXPECTILE"), ("check_dist", "DISTRIBUTIONAL"), ("check_bcq", "BCQ_THRESHOLD")])
def test_each_check_alone_refuses_every_pair_it_is_part_of(name, key):
    from video_dqn_amd import trainer
    pairs = [p for p in PAIR_TEXT if key in p]
    assert len(pairs) == 5  # the three TD keys and the two other head algorithms
    for pair in pairs:
        with pytest.raises(ValueError) as e:
            getattr(trainer, name)(_config(pair))
        assert str(e.value) == PAIR_TEXT[pair]
    getattr(trainer, name)(_config((key,)))
    getattr(trainer, name)(_config(()))


def test_rows_agree_with_the_engine_and_the_config():
    from video_dqn_amd import _lib, algos, config
    from video_dqn_amd.engine import NetEngine
    lib = _lib.load()
    assert [a.key for a in algos.ALGOS] == list(HEAD_KEYS) and [m[0] for m in algos.MODIFIERS] == ["CQL_ALPHA", "CQL_CALIBRATED", "MC_RETURN_FLOOR"]
    plain = NetEngine(3, 5, 1, True, "f32", 8, device="cpu")
    assert plain.head is None and plain.head_keys == ()
    getters = {a.head: getattr(lib, f"vdqn_net_{a.head}_head") for a in algos.ALGOS}
    defaults = config.get_cfg_defaults()
    for a in algos.ALGOS:
        net = NetEngine(3, 5, 1, True, "f32", 8, device="cpu", **{f"{a.head}_head": True})
        assert net.head == a.head and net.head_keys == a.head_keys == (f"{a.head}.weight", f"{a.head}.bias")
        assert set(net.slots) - set(plain.slots) == set(a.head_keys)
        assert {h: g(net.handle) for h, g in getters.items()} == {h: int(h == a.head) for h in getters}
        assert {h: g(plain.handle) for h, g in getters.items()} == {h: 0 for h in getters}
        assert [getattr(net, f"{b.head}_head") for b in algos.ALGOS] == [b is a for b in algos.ALGOS]
        # the statistics fit the algorithm's view of loss_stats, which starts at slot 0; the TD family needs 1 + 2 slots
        assert 1 <= len(a.stats) == len(set(a.stats)) <= algos.LOSS_SLOTS >= 3
        assert a.params[0][0] == a.key and not a.is_on(defaults) and a.is_on(_config((a.key,)))
        for key, arg, default in a.params:
            assert key in defaults and defaults[key] == default and key in config.__doc__, key
        assert hasattr(lib, a.create) and hasattr(lib, a.entry)
        assert a.kwargs(defaults) == {arg: default for _, arg, default in a.params}


def test_create_p_takes_at_most_one_head():
    from video_dqn_amd import _lib
    lib = _lib.load()
    made = []
    for vh, sh, ph in itertools.product((0, 1), repeat=3):
        cfg, h = _lib.NetConfig(3, 5, 1, 1, _lib.VDQN_F32, 8, 0), C.c_void_p()
        rc = lib.vdqn_net_create_p(C.byref(cfg), vh, sh, ph, C.byref(h))
        if rc == 0:
            made.append((vh, sh, ph))
            assert (lib.vdqn_net_value_head(h), lib.vdqn_net_spread_head(h), lib.vdqn_net_policy_head(h)) == (vh, sh, ph)
            lib.vdqn_net_destroy(h)
        else:
            assert b"out of scope" in lib.vdqn_last_error(), lib.vdqn_last_error()
    assert made == [(0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0)]
