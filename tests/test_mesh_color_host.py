"""CPU: the colour rule of transhuman_amd/mesh_color.py on a hand-made raw array (quantisation, the 128 rule, the count), and
that the point query is declared and bound."""
import numpy as np
import pytest
import torch

from transhuman_amd import mesh_color as MCol


def _logit(p):
    return float(np.log(p / (1.0 - p)))


def test_quantisation_and_the_128_rule():
    raw = torch.tensor([
        [0.0, 0.0, 0.0, 0.0],                                 # outside the hull: a zero row -> 128, counted
        [0.0, 0.0, 0.0, -3.0],                                # inside, sigma <= 0: no RGB -> 128, counted
        [_logit(0.25), _logit(0.5), _logit(0.75), 2.0],       # 63.75+.5 -> 64, 128, 191.25+.5 -> 191
        [-60.0, 60.0, _logit(100.4 / 255.0), 1e-3],           # saturates to 0 / 255; 100.4 -> 100
        [_logit(100.6 / 255.0), 0.0, 0.0, 5.0],               # 100.6 -> 101
    ], dtype=torch.float32)
    col, n = MCol.colors_from_raw(raw)
    assert col.dtype == torch.uint8 and tuple(col.shape) == (5, 3) and n == 2
    assert col.tolist() == [[128, 128, 128], [128, 128, 128], [64, 128, 191], [0, 255, 100], [101, 128, 128]]
    cf, nf = MCol.colors_from_raw(raw, as_float=True)
    assert cf.dtype == torch.float32 and nf == 2
    assert torch.equal(col, torch.clamp(torch.floor(255.0 * cf + 0.5), 0, 255).to(torch.uint8))
    assert torch.equal(cf[0], torch.full((3,), 0.5))


def test_empty_raw():
    col, n = MCol.colors_from_raw(torch.zeros((0, 4)))
    assert tuple(col.shape) == (0, 3) and col.dtype == torch.uint8 and n == 0


def test_bad_view_is_refused():
    with pytest.raises(ValueError):
        MCol.vertex_colors(None, None, np.zeros((3, 3)), faces=None, view="normal")


def test_point_query_is_declared_and_bound():
    from transhuman_amd import hip
    assert "th_eval_points" in hip.SYMBOLS and callable(hip.eval_points)
    res, args = hip.SYMBOLS["th_eval_points"]
    assert len(args) == 12                                    # ctx, frame, pts, dirs, P, raw_out, ws, bytes, pool, bytes, stats, stream
