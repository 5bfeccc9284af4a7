"""DPaRF's hyper-parameters: cfg.KNN, cfg.KNN_FREQ, cfg.KNN_DIST_ALPHA (cross_transformer.py:106, :154, :170).

K4 (transhuman_amd/csrc/k_dparf.hip) takes KNN 1..7, KNN_FREQ 1..10 and any finite KNN_DIST_ALPHA > 0:
  * a neighbour record holds seven (index, weight) pairs, and the fused kernels blend at most seven rows per sample;
  * fc_0 reads [token (192) | PE (3 + 6 KNN_FREQ)] inside a 256-column operand: 3 + 6 * 10 = 63 PE channels fit, 69 do not;
  * KNN_FREQ = 0 is refused: the reference's PositionalEncoding.forward ends in ``embed.view(x.shape[0], -1)`` of an empty
    tensor (vision_transformer.py:131-133), which the torch releases it was written for reject ("cannot reshape tensor of 0 elements
    into shape [n, -1]").  torch 2.10 infers 0 there and the reference then runs on the raw offsets alone
    (tools/gen_golden_dparf_params.py records which of the two it saw, ``freq0_runs``); the value is outside the supported 1..10
    either way.
``KNN`` and ``KNN_DIST_ALPHA`` are read per call, as the reference reads them; the octave count is the network's (``PE_relative``).
``Network()`` itself still wants cfg.KNN = 7 while it is constructed (tests/test_dropin.py pins that refusal): set cfg.KNN afterwards.
"""
import math

from .config import get_cfg

KNN_MAX, KNN_FREQ_MAX = 7, 10


def check_dparf_params(knn, n_freq, alpha):
    """-> (int knn, int n_freq, float alpha), or the refusal: ValueError for what no configuration can mean,
    NotImplementedError for what this project's kernels do not take"""
    if int(knn) != knn or int(n_freq) != n_freq:
        raise ValueError(f"KNN = {knn!r} and KNN_FREQ = {n_freq!r} must be integers")
    knn, n_freq, alpha = int(knn), int(n_freq), float(alpha)
    if knn < 1:
        raise ValueError(f"KNN = {knn}: at least one neighbouring token")
    if n_freq < 0:
        raise ValueError(f"KNN_FREQ = {n_freq}: an octave count")
    if n_freq == 0:
        raise NotImplementedError("KNN_FREQ = 0: the supported range is 1..10.  The reference's own PositionalEncoding.forward "
                                  "takes view(n, -1) of an empty tensor there (vision_transformer.py:131-133), an error in the torch "
                                  "releases it was written for")
    if not (math.isfinite(alpha) and alpha > 0.0):
        raise ValueError(f"KNN_DIST_ALPHA = {alpha}: a finite softmax temperature > 0")
    if knn > KNN_MAX:
        raise NotImplementedError(f"KNN = {knn}: the limit is {KNN_MAX}, the seven (index, weight) pairs of a neighbour record")
    if n_freq > KNN_FREQ_MAX:
        raise NotImplementedError(f"KNN_FREQ = {n_freq}: the limit is {KNN_FREQ_MAX}, 63 PE channels inside fc_0's 256 padded "
                                  f"columns (192 + 3 + 6 * {n_freq} = {195 + 6 * n_freq})")
    return knn, n_freq, alpha


def check_centres(knn, n_centres):
    """fewer than KNN token centres is an error (pytorch3d's knn_points would hand back padded neighbours)"""
    if int(n_centres) < int(knn):
        raise ValueError(f"need at least {int(knn)} token centres (KNN), got {int(n_centres)}")


def params_in_force(net, cfg=None):
    """(cfg.KNN, net.PE_relative.num_freqs, cfg.KNN_DIST_ALPHA), checked: what every entry that runs K4 hands to hip.set_dparf"""
    cfg = cfg or get_cfg()
    return check_dparf_params(cfg.KNN, net.PE_relative.num_freqs, cfg.KNN_DIST_ALPHA)
