"""cfg.train_encoder_fwd and the C ABI of K29 on the host: the key's default, its absence from TRAIN_SWITCHES and its checked reader;
the key is read only under cfg.train_encoder = "device"; th_conv2d_fwd32_supported answers 1 for exactly the trunk's five
convolutions; the tile and chunk queries; the entry points are declared, exported and bound; null pointers and unsupported shapes
are refused before any device is touched."""
from types import SimpleNamespace

import pytest
import torch

from transhuman_amd import config
from transhuman_amd.config import get_cfg, override
from transhuman_amd.networks import autograd_path, train_ops

ENTRIES = ("th_conv2d_fwd32_supported", "th_conv2d_fwd32_tile_rows", "th_conv2d_fwd32_tile_cols", "th_conv2d_fwd32_chunk_channels",
           "th_conv2d_fwd32")
SHAPES = ((3, 64, 7, 2), (64, 64, 3, 1), (64, 128, 3, 2), (64, 128, 1, 2), (128, 128, 3, 1))      # cin cout ks stride


@pytest.fixture(scope="module")
def lib():
    from transhuman_amd import build, hip
    build.build(force=False, verbose=False)
    return hip.load_library()


def test_key_default_table_and_reader():
    assert config.TRAIN_ENCODER_FWD == ("torch", "device") and "train_encoder_fwd" not in config.TRAIN_SWITCHES
    assert len(config.TRAIN_SWITCHES) == 7
    assert config._defaults().train_encoder_fwd == "torch" and get_cfg().train_encoder_fwd == "torch"
    assert autograd_path.encoder_fwd_mode() == "torch"
    assert autograd_path.encoder_fwd_mode("torch") == "torch" and autograd_path.encoder_fwd_mode("device") == "device"
    for bad in ("Device", "", "hip", "miopen", 1):
        with pytest.raises(ValueError, match="cfg.train_encoder_fwd must be 'torch' or 'device'"):
            autograd_path.encoder_fwd_mode(bad)
    with override(train_encoder_fwd="device"):
        assert autograd_path.encoder_fwd_mode() == "device" and train_ops._encoder_fwd() == "device"
    with override(train_encoder_fwd="fast"), pytest.raises(ValueError, match="train_encoder_fwd"):
        autograd_path.encoder_fwd_mode()
    assert get_cfg().train_encoder_fwd == "torch"


def test_a_cfg_without_the_key_means_torch(monkeypatch):
    """the reference's cfg has none of the train_* keys"""
    monkeypatch.setattr(autograd_path, "get_cfg", lambda: SimpleNamespace())
    assert autograd_path.encoder_fwd_mode() == "torch"


def test_key_is_read_only_under_the_device_encoder():
    """under train_encoder = "torch" a bad value raises nothing, like train_gather_bwd under "full"; under "device" a CPU batch
    is refused by the existing rule whatever the key says"""
    from transhuman_amd import hip
    from transhuman_amd.networks.encoder import SpatialEncoder
    torch.manual_seed(0)
    enc = SpatialEncoder().train()
    img = torch.randn(1, 3, 16, 16)
    with override(train_encoder_fwd="torch"):
        want = [l.detach().clone() for l in autograd_path._trunk(SpatialEncoder().train().requires_grad_(False), img, "torch")]
    for value in ("sorted", "device"):
        with override(train_encoder="torch", train_encoder_fwd=value):
            got = autograd_path._trunk(enc, img, "torch")
            assert len(got) == len(want) == 3
        batch = {"ray_o": torch.zeros(1, 4, 3), "ray_d": torch.ones(1, 4, 3)}
        with override(train_encoder="torch", train_encoder_fwd=value):
            with pytest.raises(Exception) as e:
                autograd_path.render(SimpleNamespace(net=None), batch)
        assert "train_encoder_fwd" not in str(e.value)
        with override(train_encoder="device", train_encoder_fwd=value), pytest.raises(hip.HipError, match="MI355X"):
            autograd_path.trunk_device(enc, img)
    x = torch.zeros(1, 64, 4, 4, requires_grad=True)
    w = torch.zeros(64, 64, 3, 3, requires_grad=True)
    bn = torch.nn.BatchNorm2d(64).train()
    with override(train_encoder_fwd="device"):
        for call in (lambda: train_ops.ConvFn.apply(x, w, 1), lambda: train_ops.MaxPoolFn.apply(x),
                     lambda: train_ops.BnActFn.apply(x, bn, None, True, bn.weight, bn.bias)):
            with pytest.raises(hip.HipError):
                call()
    assert int(bn.num_batches_tracked) == 0


def test_entry_points_declared_exported_bound(lib):
    from transhuman_amd import hip
    for name in ENTRIES:
        assert name in hip.SYMBOLS and hasattr(lib, name), name
    assert len(hip.SYMBOLS["th_conv2d_fwd32"][1]) == 12
    assert lib.th_abi_version() == 12


def test_supported_is_exactly_the_five_shapes(lib):
    from transhuman_amd import hip
    for s in SHAPES:
        assert lib.th_conv2d_fwd32_supported(*s) == 1 and hip.conv2d_fwd32_supported(*s) is True, s
    n = 0
    for cin in (0, 1, 3, 32, 64, 128, 256):
        for cout in (0, 3, 64, 128, 256):
            for ks in (0, 1, 3, 5, 7):
                for stride in (0, 1, 2, 3):
                    got = lib.th_conv2d_fwd32_supported(cin, cout, ks, stride)
                    assert got == int((cin, cout, ks, stride) in SHAPES), (cin, cout, ks, stride)
                    n += got
    assert n == 5
    for bad in ((3, 64, 3, 1), (64, 64, 5, 1), (64, 64, 3, 2), (128, 64, 3, 1), (64, 128, 1, 1), (-64, 64, 3, 1)):
        assert hip.conv2d_fwd32_supported(*bad) is False


def test_tile_and_chunk_queries(lib):
    from transhuman_amd import hip
    rows, cols = hip.conv2d_fwd32_tile()
    assert rows == lib.th_conv2d_fwd32_tile_rows() > 0 and cols == lib.th_conv2d_fwd32_tile_cols() > 0
    ck = hip.conv2d_fwd32_chunk_channels()
    assert ck == lib.th_conv2d_fwd32_chunk_channels() > 0
    assert 64 % ck == 0 and 128 % ck == 0                       # every trunk shape but conv1 is a whole number of chunks


def test_refusals_reach_no_device(lib):
    """a null context or pointer is a negative status with a message, before anything is launched"""
    import ctypes
    from transhuman_amd import hip
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.th_conv2d_fwd32(None, p, 1, 64, 4, 4, p, 64, 3, 1, p, None) < 0
    assert b"th_conv2d_fwd32" in lib.th_last_error()
    with pytest.raises(ValueError, match="conv2d_fwd32"):
        hip.conv2d_fwd32(torch.zeros(1, 64, 4, 4), torch.zeros(64, 64, 3, 3), 1)
