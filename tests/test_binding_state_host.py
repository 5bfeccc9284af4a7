"""The binding's bookkeeping that needs neither the library nor a device: which slots of a range table trip which switch
(hip.range_trips), the resolver from a device argument to the per-device record (hip._state), and the defaults of the caller's
modes on a host without a GPU."""
import pytest
import torch

from transhuman_amd import hip

LIMIT, FLOOR, LIMIT32 = hip.RANGE_FP16_LIMIT, hip.RANGE_FP16_FLOOR, hip.RANGE_FP32_LIMIT
NONE_SET = {"mlp": False, "conv": False, "vit": False}


def _table(**slots):
    return [slots.get(name, 0) for name in hip.RANGE_NAMES]


def _kinds(vals, flags=NONE_SET):
    return [kind for kind, _ in hip.range_trips(vals, flags)]


def test_an_all_zero_table_trips_nothing():
    """0 is "slot never written", not "below the floor" """
    assert hip.range_trips([0] * 8, NONE_SET) == []


@pytest.mark.parametrize("name", hip.RANGE_NAMES[:6])
def test_mlp_slots(name):
    (kind, text), = hip.range_trips(_table(**{name: LIMIT}), NONE_SET)
    assert kind == "mlp" and f"{name}: " in text and "fp16 hi/lo split" in text and "reached the fp16 limit" in text
    assert _kinds(_table(**{name: LIMIT - 1})) == []
    (kind, text), = hip.range_trips(_table(**{name: FLOOR - 1}), NONE_SET)
    assert kind == "mlp" and f"{name}: " in text and "below 2^-6" in text
    assert _kinds(_table(**{name: FLOOR})) == []
    assert _kinds(_table(**{name: 0x7c00})) == ["mlp"] and _kinds(_table(**{name: 0x7e00})) == ["mlp"]     # inf, NaN


def test_conv_slot():
    (kind, text), = hip.range_trips(_table(conv_in=LIMIT32), NONE_SET)
    assert kind == "conv" and "convolution" in text
    assert _kinds(_table(conv_in=LIMIT32 - 1)) == []


def test_transhe_slot():
    (kind, text), = hip.range_trips(_table(vit_in=LIMIT), NONE_SET)
    assert kind == "vit" and "TransHE" in text
    assert _kinds(_table(vit_in=LIMIT - 1)) == []
    assert _kinds(_table(vit_in=FLOOR - 1)) == [] and _kinds(_table(vit_in=1)) == []      # (no floor rule for this slot)


def test_order_and_switches_already_set():
    vals = _table(inter=LIMIT, conv_in=LIMIT32, vit_in=LIMIT)
    assert _kinds(vals) == ["vit", "conv", "mlp"]
    for kind in NONE_SET:
        assert _kinds(vals, {**NONE_SET, kind: True}) == [k for k in ("vit", "conv", "mlp") if k != kind]
    assert _kinds(vals, {"mlp": True, "conv": True, "vit": True}) == []


def test_resolver_finds_one_record_per_device(monkeypatch):
    monkeypatch.setattr(hip, "_states", {})
    st = hip._state(1)
    assert st.index == 1
    for device in ("cuda:1", torch.device("cuda", 1), torch.device("cuda:1")):
        assert hip._state(device) is st
    assert hip._state(2) is not st and hip._state("cuda:2") is hip._state(2)
    assert st.handle is None and hip._state(2).handle is None            # (looking a record up creates no context)


@pytest.mark.parametrize("env,want", ((None, 8), ("4", 4), ("8", 8)))
def test_fused_waves_default(monkeypatch, env, want):
    monkeypatch.setattr(hip, "_states", {})
    if env is None:
        monkeypatch.delenv("TH_FUSED_WAVES", raising=False)
    else:
        monkeypatch.setenv("TH_FUSED_WAVES", env)
    assert hip.fused_waves() == want
    assert hip._states == {}


@pytest.mark.parametrize("env,want", ((None, True), ("0", False), ("1", True)))
def test_tex_rows_default(monkeypatch, env, want):
    monkeypatch.setattr(hip, "_states", {})
    if env is None:
        monkeypatch.delenv("TH_ROWS_TEX", raising=False)
    else:
        monkeypatch.setenv("TH_ROWS_TEX", env)
    assert hip.tex_rows_enabled() is want
    assert hip._states == {}
