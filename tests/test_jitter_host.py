"""CPU: the colour jitter of the raw frames (transhuman_amd/preprocess.py, K25) -- the numpy restatement ``color_jitter_oracle``
against Pillow byte for byte (ImageEnhance.Brightness / Contrast / Color for the three blends, convert("HSV") / convert("RGB") around
an addition to the H plane for the hue, and the whole chain in all 24 orders), ``jitter_params`` against the same draws made on the
global generator, the configuration key and the exported symbols.  torchvision is absent: what is pinned here is the image
arithmetic of Pillow, on which torchvision's PIL path rests; its choice of draws is followed from its documentation."""
import itertools

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

from transhuman_amd import preprocess as pp
from transhuman_amd.config import _defaults, get_cfg, override

FACTORS = (0.2, 0.3, 0.5, 1.0, 1.37, 2.0)
ENHANCERS = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)
IDENTITY = (0, 1, 2, 3)


def images():
    """a random 37 x 53 image, a low-contrast one and a constant one"""
    rng = np.random.default_rng(25)
    return dict(random=rng.integers(0, 256, (37, 53, 3), dtype=np.uint8),
                low=(118 + rng.integers(0, 9, (37, 53, 3))).astype(np.uint8),
                constant=np.broadcast_to(np.array([200, 31, 97], np.uint8), (37, 53, 3)).copy())


def only(op, value):
    """the parameter set that runs one operation"""
    factors = [None] * 4
    factors[op] = value
    return pp.JitterParams(IDENTITY, *factors)


def cube(stride=3):
    """the colour cube of that stride plus 255 per channel, as one [n, n * n, 3] image"""
    c = np.unique(np.append(np.arange(0, 256, stride), 255)).astype(np.uint8)
    return np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(len(c), len(c) * len(c), 3)


def pil_hue(img, d):
    """Pillow's conversions around the addition to the H plane (what torchvision's PIL path does)"""
    hsv = np.array(Image.fromarray(img).convert("HSV"))
    hsv[..., 0] += np.uint8(d)                                          # (wraps)
    return np.asarray(Image.fromarray(hsv, "HSV").convert("RGB"))


def pil_chain(img, params):
    order, *factors = params
    im = Image.fromarray(img)
    for op in order:
        if factors[op] is None:
            continue
        if op == pp.HUE:
            im = Image.fromarray(pil_hue(np.asarray(im), pp.hue_shift(factors[op])))
        else:
            im = ENHANCERS[op](im).enhance(factors[op])
    return np.asarray(im)


@pytest.mark.parametrize("op", [pp.BRIGHTNESS, pp.CONTRAST, pp.SATURATION])
@pytest.mark.parametrize("name", ["random", "low", "constant"])
def test_each_blend_equals_pillow(op, name):
    img = images()[name]
    for f in FACTORS:
        ref = np.asarray(ENHANCERS[op](Image.fromarray(img)).enhance(f))
        got = pp.color_jitter_oracle(img, only(op, f))
        assert got.dtype == np.uint8 and got.shape == img.shape
        assert np.array_equal(got, ref), (op, name, f, int(np.abs(got.astype(int) - ref).max()))
    assert not np.array_equal(pp.color_jitter_oracle(images()["random"], only(op, 0.3)), images()["random"])


def test_hue_equals_pillow_on_the_colour_cube():
    img = cube()
    assert img.shape == (86, 86 * 86, 3)
    for d in (0, 1, 77, 128, 255):                                      # (128 is no trunc(255 h) of a hue in [-0.5, 0.5]: the shift itself)
        want = pil_hue(img, d)
        assert np.array_equal(pp.hue_oracle(img.astype(np.int64), d), want), d
        if d != 128:
            h = (d + 0.5) / 255.0 if d < 128 else (d - 256 - 0.5) / 255.0
            assert pp.hue_shift(h) == d, (d, h)
            assert np.array_equal(pp.color_jitter_oracle(img, only(pp.HUE, h)), want), d
    # the shift of a negative hue: truncation towards zero, then mod 256
    assert pp.hue_shift(-0.5) == 129 and pp.hue_shift(0.5) == 127 and pp.hue_shift(-0.001) == 0 and pp.hue_shift(-0.3) == 256 - 76
    assert np.array_equal(pp.color_jitter_oracle(img, only(pp.HUE, -0.3)), pil_hue(img, 180))
    # d = 0 is no identity: the round trip through the integer HSV is lossy
    assert not np.array_equal(pp.color_jitter_oracle(img, only(pp.HUE, 0.0)), img)


def test_all_orders_equal_the_pillow_chain():
    img = np.random.default_rng(3).integers(0, 256, (16, 16, 3), dtype=np.uint8)
    seen = set()
    for order in itertools.permutations(range(4)):
        params = pp.JitterParams(order, 1.4, 0.6, 1.7, -0.21)
        got = pp.color_jitter_oracle(img, params)
        assert np.array_equal(got, pil_chain(img, params)), order
        seen.add(got.tobytes())
    assert len(seen) > 12                                               # the order matters


def test_images_of_a_stack_get_their_own_contrast_mean():
    rng = np.random.default_rng(4)
    stack = np.stack([rng.integers(lo, lo + 60, (9, 11, 3)) for lo in (0, 90, 190)]).astype(np.uint8)
    params = pp.JitterParams((0, 2, 1, 3), 1.1, 0.4, 1.3, 0.1)
    got = pp.color_jitter_oracle(stack, params)
    for v in range(3):
        assert np.array_equal(got[v], pil_chain(stack[v], params)), v
    assert np.array_equal(pp.color_jitter_oracle(stack[1], params), got[1])                       # [H,W,3]
    assert np.array_equal(pp.color_jitter_oracle(stack[None], tuple(params)), got[None])          # more leading dimensions, a plain tuple


def test_jitter_params_are_the_draws_of_the_documented_get_params():
    torch.manual_seed(99)
    state = torch.get_rng_state()
    for seed in (0, 7, 123456789):
        p = pp.jitter_params(seed)
        assert torch.equal(torch.get_rng_state(), state)                # the global generator: neither reseeded nor advanced
        torch.manual_seed(seed)
        order = tuple(int(i) for i in torch.randperm(4))
        b, c, s, h = (float(torch.empty(1).uniform_(lo, hi)) for lo, hi in ((0.2, 2), (0.3, 2), (0.2, 2), (-0.5, 0.5)))
        assert p == (order, b, c, s, h) and isinstance(p.order, tuple) and sorted(p.order) == [0, 1, 2, 3]
        assert 0.2 <= p.brightness <= 2 and 0.3 <= p.contrast <= 2 and 0.2 <= p.saturation <= 2 and -0.5 <= p.hue <= 0.5
        torch.set_rng_state(state)
    assert pp.jitter_params(5) == pp.jitter_params(5) != pp.jitter_params(6)
    assert pp.jitter_params(torch.tensor(5)) == pp.jitter_params(5)
    # a range given as None switches that operation off, its slot in the order stays, and no draw is made for it
    torch.manual_seed(11)
    order = tuple(int(i) for i in torch.randperm(4))
    b, s = (float(torch.empty(1).uniform_(lo, hi)) for lo, hi in ((0.5, 1.5), (0.2, 2)))
    torch.set_rng_state(state)
    p = pp.jitter_params(11, brightness=(0.5, 1.5), contrast=None, hue=None)
    assert p == (order, b, None, s, None)
    img = images()["random"]
    off = pp.color_jitter_oracle(img, p)
    assert np.array_equal(off, pil_chain(img, p))
    assert np.array_equal(pp.color_jitter_oracle(img, pp.JitterParams(IDENTITY, None, None, None, None)), img)


def test_arguments_are_checked():
    img = images()["random"]
    with pytest.raises(TypeError, match="uint8"):
        pp.color_jitter_oracle(img.astype(np.float32) / 255, only(0, 1.2))
    with pytest.raises(ValueError, match="order"):
        pp.color_jitter_oracle(img, ((0, 1, 2, 2), 1.0, 1.0, 1.0, 0.0))
    with pytest.raises(ValueError, match="brightness"):
        pp.color_jitter_oracle(img, only(0, -0.1))
    with pytest.raises(ValueError, match="contrast"):
        pp.color_jitter_oracle(img, only(1, float("nan")))
    with pytest.raises(ValueError, match="hue"):
        pp.color_jitter_oracle(img, only(3, 0.6))
    with pytest.raises(ValueError, match="shape"):
        pp.color_jitter_oracle(img[..., :2], only(0, 1.2))
    with pytest.raises(TypeError, match="uint8"):                       # checked before any device is asked for
        pp.color_jitter(img.astype(np.int32), only(0, 1.2))


def test_configuration_key():
    assert _defaults().input_jitter == "batch" and get_cfg().input_jitter == "batch"
    from transhuman_amd.config import TRAIN_SWITCHES
    assert "input_jitter" not in TRAIN_SWITCHES
    batch = {"jitter_seed": 41}
    assert pp.batch_jitter(batch) is None                               # "batch": the seed is ignored
    with override(input_jitter="device"):
        assert pp.batch_jitter(batch) == pp.jitter_params(41)
        assert pp.batch_jitter({"jitter_seed": torch.tensor([41])}) == pp.jitter_params(41)
        assert pp.batch_jitter({}) is None                              # no seed (the test split): not jittered
        with pytest.raises(TypeError, match="jitter_seed"):
            pp.batch_jitter({"jitter_seed": torch.tensor(0.5)})
    with override(input_jitter="host"), pytest.raises(ValueError, match="input_jitter"):
        pp.batch_jitter(batch)
    # the reference's own key is not read: it keeps meaning that the dataset did it
    with override(jitter=True):
        assert pp.batch_jitter(batch) is None
    assert get_cfg().input_jitter == "batch" and batch == {"jitter_seed": 41}


def test_the_library_exports_both_symbols():
    from transhuman_amd import hip
    lib = hip.load_library()
    assert "th_color_jitter" in hip.SYMBOLS and "th_color_jitter_workspace_bytes" in hip.SYMBOLS
    ws = lib.th_color_jitter_workspace_bytes
    assert lib.th_color_jitter is not None and ws(4, 1024, 1024) == 4 * 256 * 8
    assert ws(1, 1, 1) >= 8 and ws(3, 16384, 16384) == 3 * 1024 * 8 and ws(1, 0, 5) == 0 and ws(70000, 4, 4) == 0
