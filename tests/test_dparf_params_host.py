"""cfg.KNN 1..7, cfg.KNN_FREQ 1..10, any cfg.KNN_DIST_ALPHA > 0, without a GPU: construction and refusals, checkpoints of every
fc_0 width, the training entry on "torch" against the reference's recorded step, the oracle against the recordings
(tests/golden/g28_dparf_params*.npz, tools/gen_golden_dparf_params.py), and point_network_device's padding at every width."""
import functools
import os

import numpy as np
import pytest
import torch

import dparf_params_case as C
from oracle import th_oracle as O
from train_step_case import STEP_CFG, check_step, setup
from transhuman_amd import config, synth
from transhuman_amd.dparf_params import check_centres, check_dparf_params
from transhuman_amd.networks import autograd_path
from transhuman_amd.networks.cross_transformer import Network
from util import GOLD, can_centres64, csr, maxdiff, synth_assign


# ---- construction and refusals -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", list(C.TRIPLES))
def test_network_is_built_under_every_triple(t):
    K, F_, alpha = C.TRIPLES[t]
    with config.override(vit_depth=2, **C.build_cfg(t)):
        net = Network()
    assert tuple(net.fc_0.weight.shape) == (256, 195 + 6 * F_, 1)
    assert net.PE_relative.num_freqs == F_ and net.PE_relative.d_out == 3 + 6 * F_
    assert check_dparf_params(K, F_, alpha) == (K, F_, alpha)


@pytest.mark.parametrize("knn", range(1, 8))
@pytest.mark.parametrize("n_freq", [1, 10])
def test_the_whole_range_is_accepted(knn, n_freq):
    assert check_dparf_params(knn, n_freq, 1e-3) == (knn, n_freq, 1e-3)
    assert check_dparf_params(knn, n_freq, 1e30)[2] == 1e30


def test_refusals():
    def refused(exc, match, **keys):
        with config.override(vit_depth=2, **keys):
            with pytest.raises(exc, match=match):
                Network()
    refused(NotImplementedError, r"KNN = 8: the limit is 7, the seven \(index, weight\) pairs", KNN=8)
    refused(NotImplementedError, "KNN = 5 at construction.*read on every call", KNN=5)     # (per call: 1..7, below)
    refused(NotImplementedError, r"KNN_FREQ = 11: the limit is 10, 63 PE channels inside fc_0's 256 padded", KNN_FREQ=11)
    refused(NotImplementedError, r"KNN_FREQ = 0.*PositionalEncoding\.forward.*view\(n, -1\) of an empty", KNN_FREQ=0)
    refused(ValueError, "KNN = 0", KNN=0)
    refused(ValueError, "KNN_FREQ = -1", KNN_FREQ=-1)
    for a in (0.0, -0.5, float("inf"), float("nan")):
        refused(ValueError, "KNN_DIST_ALPHA", KNN_DIST_ALPHA=a)
    refused(ValueError, "integers", KNN=2.5)
    with config.override(vit_depth=2):
        Network()                                                  # (and the defaults still build)


def test_fewer_centres_than_neighbours_is_an_error():
    check_centres(3, 3)
    with pytest.raises(ValueError, match="at least 3 token centres .*got 2"):
        check_centres(3, 2)
    # Network.forward says so before anything reaches the device; KNN is read per call
    with config.override(vit_depth=2):
        net = Network()
    dd = {"pts_smplcoord": torch.zeros(1, 5, 3), "obs_smpl_smplcoord": torch.zeros(1, 2, 3), "blend_mtx": torch.eye(4).repeat(1, 2, 1, 1)}
    with config.override(KNN=3):
        with pytest.raises(ValueError, match="at least 3 token centres"):
            net(torch.zeros(3, 384, 5), torch.zeros(1, 5, 27), dd, holder=torch.zeros(3, 2, 192))


# ---- a reference checkpoint of every width ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_freq", [1, 4, 6, 10])
def test_checkpoint_round_trip(n_freq):
    with config.override(vit_depth=2, KNN_FREQ=n_freq):
        net, other = Network(), Network()
    sd = synth.det_state_dict(net.state_dict(), seed=3, sigma_bias=-1.7)
    assert tuple(sd["fc_0.weight"].shape) == (256, 195 + 6 * n_freq, 1)
    sd["xyzc_net.conv0.0.weight"] = torch.zeros(3, 3, 3, 192, 64)          # the reference's dead sub-module
    other.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, other.state_dict()[k]) for k, v in sd.items() if not k.startswith("xyzc_net."))
    with config.override(vit_depth=2, KNN_FREQ=n_freq % 10 + 1):
        wrong = Network()
    with pytest.raises(RuntimeError, match="fc_0.weight"):
        wrong.load_state_dict(sd, strict=True)


# ---- the training entry, every switch on "torch" -----------------------------------------------------------------------------------
def test_torch_training_step_reproduces_the_reference_under_B():
    """g18's bars (train_step_case.check_step): outputs 2e-5, loss 1e-6, the 20 gradients 2e-3 of their maximum"""
    with config.override(**STEP_CFG, **C.build_cfg("B")):
        net, r, b = setup("cpu")
        assert net.fc_0.weight.shape[1] == 231
        with C.under("B"):                                          # (KNN: per call)
            check_step(C.step_recording("B"), net, r, b)


# ---- the oracle against the recordings -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", list(C.TRIPLES))
def test_oracle_rows_equal_the_recording(t):
    K, F_, alpha = C.TRIPLES[t]
    g7 = np.load(os.path.join(GOLD, "g7_dparf.npz"))
    tok = torch.from_numpy(np.load(os.path.join(GOLD, "g6_vit.npz"))["out"])
    ref = torch.from_numpy(C.golden()[f"rep_{t}"]).permute(2, 0, 1)                              # [P,V,195 + 6 F]
    out = O.dparf(torch.from_numpy(g7["pts_s"]), torch.from_numpy(g7["centres"]), torch.from_numpy(g7["blend"]), tok, K=K,
                  n_freq=F_, alpha=alpha)
    assert out.shape == ref.shape == (256, 3, 195 + 6 * F_)
    assert maxdiff(out, ref) <= 2e-6 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("t", list(C.TRIPLES))
def test_oracle_forward_equals_the_recording(t):
    """the bar tests/test_oracle_golden.py holds g8 to"""
    K, F_, alpha = C.TRIPLES[t]
    g = C.golden()
    pf, vd, pts, mask, centres, blend, tok = C.forward_inputs()
    sd = {k: v.detach() for k, v in C.make_net(t).state_dict().items()}
    fwd = functools.partial(O.network_forward, K=K, n_freq=F_, alpha=alpha)
    assert maxdiff(fwd(sd, pf, vd, pts, centres, blend, tok, None), torch.from_numpy(g[f"fwd_{t}_none"])) < 2e-5
    assert maxdiff(fwd(sd, pf, vd, pts, centres, blend, tok, mask), torch.from_numpy(g[f"fwd_{t}_rand"])) < 2e-5
    if t == "B":
        assert maxdiff(fwd(sd, pf[:1], vd, pts, centres, blend, tok[:1], None), torch.from_numpy(g["fwd_B_v1_none"])) < 2e-5
        assert maxdiff(fwd(sd, pf[:1], vd, pts, centres, blend, tok[:1], mask), torch.from_numpy(g["fwd_B_v1_rand"])) < 2e-5


@pytest.mark.parametrize("t", ["B", "D"])
def test_oracle_frame_equals_the_recording(t, monkeypatch):
    """the bars of tests/test_oracle_golden.py for g11_render_small; O.render_fast calls O.network_forward with its defaults"""
    K, F_, alpha = C.TRIPLES[t]
    g = C.golden()
    monkeypatch.setattr(O, "network_forward", functools.partial(O.network_forward, K=K, n_freq=F_, alpha=alpha))
    b = synth.make_batch(32, 32, 3, seed=0)
    sd = {k: v.detach() for k, v in C.make_net(t).state_dict().items()}
    hol, pix = O.encoder_forward(sd, b["input_imgs"][0][0])
    off, mem = csr(synth_assign(300))
    out, _ = O.render_fast(sd, b, hol, pix, off, mem, can_centres64(synth_assign(300)), n_samples=32)
    assert maxdiff(out["rgb_map"][0], torch.from_numpy(g[f"frame_{t}_rgb"])) < 2e-5
    assert maxdiff(out["acc_map"][0], torch.from_numpy(g[f"frame_{t}_acc"])) < 2e-5
    assert maxdiff(out["depth_map"][0], torch.from_numpy(g[f"frame_{t}_depth"])) < 1e-4


# ---- point_network_device pads fc_0 from its own width -----------------------------------------------------------------------------
@pytest.mark.parametrize("n_freq", [1, 4, 6, 10])
def test_point_network_device_equals_point_network_at_every_width(n_freq):
    width = 195 + 6 * n_freq
    assert width in (201, 219, 231, 255)
    with config.override(vit_depth=2, KNN_FREQ=n_freq):
        torch.manual_seed(0)
        net = Network().double()
    rs = np.random.RandomState(n_freq)
    P, V = 37, 3
    h = torch.from_numpy(rs.normal(size=(P, V, width)))
    f = torch.from_numpy(rs.normal(size=(P, V, 384)))
    vd = torch.from_numpy(rs.normal(size=(P, 27)))
    with torch.no_grad():
        ref = autograd_path.point_network(net, h, f, vd)
        got = autograd_path.point_network_device(net, h, f, vd, ops=autograd_path.point_network_torch_ops())
        padded = autograd_path.point_network_device(net, torch.nn.functional.pad(h, (0, 256 - width)), f, vd,
                                                    ops=autograd_path.point_network_torch_ops())
    assert maxdiff(got, ref) < 1e-12 and maxdiff(padded, ref) < 1e-12
