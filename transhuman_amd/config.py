"""Mirror of the ~20 configuration keys the rendering hot path reads.

The reference builds a global yacs ``cfg`` at import time
(/root/reference/lib/config/config.py:152-167) from
configs/train_or_eval.yaml.  The hot path only reads the keys listed in
SURVEY.md section 5 ("Config / flags").  When this package is used as a
drop-in inside the reference tree (``lib.config`` already imported by run.py)
we bind to that very object so YAML/CLI overrides keep working; standalone we
use a plain namespace carrying the same defaults
(configs/train_or_eval.yaml:16-127).
"""
import sys
from contextlib import contextmanager
from types import SimpleNamespace

# the switches of the training entry (autograd_path.render reads them in this order): key -> its allowed values.  The first
# value is the default in _defaults() below, and the one a CPU batch can run
TRAIN_SWITCHES = {
    "train_kernels": ("torch", "device"),
    "train_attention": ("torch", "device"),
    "train_vit_dense": ("torch", "device"),
    "train_maps": ("full", "latents"),
    "train_gather_bwd": ("atomic", "ordered"),
    "train_point_net": ("torch", "device"),
    "train_encoder": ("torch", "device"),
}


TRAIN_SYNC_BN = ("torch", "device")

# cfg.train_encoder_fwd: the forward of the trunk's sites under train_encoder = "device".  Not a row of TRAIN_SWITCHES either: it
# selects nothing unless that switch is on its device value (autograd_path.encoder_fwd_mode is its reader)
TRAIN_ENCODER_FWD = ("torch", "device")


def _defaults():
    return SimpleNamespace(
        # sampling / compositing (train_or_eval.yaml:17-43, run.py:22)
        N_samples=64,
        perturb=0.0,
        raw_noise_std=0.0,
        white_bkgd=False,
        run_mode="test",
        H=1024,
        W=1024,
        ratio=0.5,
        # painting (train_or_eval.yaml:24,41-42,47)
        time_steps=1,
        rasterize=True,
        depth_map=False,
        depth_vizmap=False,
        # where the vertex mask of painting comes from: "batch" (input_vizmaps, as the reference) or "device" (rasterised here
        # from input_smpl_vertice, the input cameras and the renderer's faces; transhuman_amd/visibility.py)
        vizmap_source="batch",
        # where batch['input_imgs'] / batch['input_K'] come from: "batch" (as the reference: its dataset prepares them on the host)
        # or "device" (made here from the raw camera frames input_imgs_raw / input_msks_raw / input_K_raw / input_D: undistort,
        # resize by `ratio`, background under the mask; transhuman_amd/preprocess.py, Renderer.frame_inputs)
        input_prep="batch",
        # who applies the training colour jitter to the raw frames: "batch" (as the reference: its dataset did, or did not, before
        # the frames got here; nothing is done) or "device" (a batch that carries `jitter_seed` -- the reference's
        # index + epoch * cfg.seed -- gets input_imgs_raw and target_img_raw jittered in front of their preparation: read only
        # where input_prep / target_prep = "device" prepare a raw frame; transhuman_amd/preprocess.py, K25).  This is not the
        # reference's own `jitter` key, which keeps meaning that its dataset does it
        input_jitter="batch",
        # architecture (train_or_eval.yaml:51-56)
        embed_size=192,
        img_feat_size=384,
        xyz_res=10,
        view_res=4,
        pretrained=False,
        # TransHE / DPaRF (train_or_eval.yaml:58-68)
        num_class=300,
        vit_depth=12,
        KNN=7,
        KNN_FREQ=10,
        KNN_DIST_ALPHA=0.5,
        KNN_SIGMA=0.25,
        use_truncation=False,
        # mesh (configs/reconstruction.yaml:14-15)
        voxel_size=[0.005, 0.005, 0.005],
        mesh_th=20,
        # what if_mesh_renderer.Renderer.render does to the mesh it returns (never to `cube`): mesh_components = "all" (as the
        # reference: floaters included), "largest" or an int n (every component with >= n faces; mesh_clean.py, K24), then
        # mesh_colors = "none" (as the reference: no colours) or "normal" (the field's RGB at every vertex, looked at against the
        # vertex normal; mesh_color.py, th_eval_points)
        mesh_components="all",
        mesh_colors="none",
        exp_name="transhuman_amd",
        data_root="data/zju_mocap",
        # where the kmeans CSR fixtures live when ./kmeans_dict is absent
        kmeans_dir=None,
        # hull distance and small-frame switch are literals in the reference
        # (if_clight_renderer.py:442 and :551); kept here as named constants
        hull_dist=0.1,
        small_frame_rays=2400,
        chunk_points=1024 * 32,
        # the training entry (autograd_path.render): "torch" composes every stage from torch operators; "device" runs the token
        # blend, the pixel-aligned gather and the compositing through the HIP forwards with HIP adjoints (networks/train_ops.py)
        train_kernels="torch",
        # the attention of TransHE's blocks in the training entry: "torch" builds q k^T, softmax and the product with v from torch
        # operators (autograd keeps the [V,heads,N,N] probabilities of every layer); "device" runs the inference path's attention
        # kernels with the HIP backward that recomputes them tile by tile (train_ops.AttentionFn)
        train_attention="torch",
        # everything else inside TransHE's blocks in the training entry -- the dense layers, LayerNorm and GELU: "torch" runs the
        # torch modules under torch autograd; "device" runs the fp32 MFMA GEMMs with HIP backwards that recompute LN(x) and gelu(u)
        # and add their partial sums in a fixed order (train_ops.NormLinearFn / LinearFn / GeluLinearFn / LayerNormFn)
        train_vit_dense="torch",
        # what the training entry samples its image features from: "full" builds the reference's two full-size maps (pixel_feat_map
        # [V,384,H,W], holder_feat_map [V,192,H,W]) and their gradients; "latents" samples the encoder's three latents and the
        # images directly at the vertices and the ray samples (train_ops.LatentGatherFn, K19) -- neither map exists
        train_maps="full",
        # the adjoint of that gather, read only with train_maps = "latents": "atomic" clears the three latent gradients and adds
        # onto them with float atomics (last bits differ from run to run; the lift's gradient through torch's GEMM); "ordered"
        # sorts the (sample, view) pairs by map pixel and sums per latent texel in ascending (row, column, sample, slot) order,
        # the lift's gradient by fixed-order partial sums -- all five gradients bit-identical from run to run
        # (th_latent_gather_bwd_ordered, k_latgather_ord.hip)
        train_gather_bwd="atomic",
        # the per-point network (MLP_forward_ori) in the training entry: "torch" composes it from torch operators under torch
        # autograd; "device" runs it layer by layer on the fp32 MFMA GEMMs of the inference path with HIP backwards
        # (autograd_path.point_network_device: train_ops.ReluLinearFn / LinearFn / CrossViewAttentionFn, K20)
        train_point_net="torch",
        # the ResNet18 trunk of the encoder (conv1 / bn1, the max pool, layer1, layer2) in the training entry: "torch" runs the stock
        # modules under torch autograd; "device" runs the same torch operators in the forward, site by site without a graph, and
        # HIP backwards with fixed-order sums (autograd_path.trunk_device: train_ops.ConvFn / BnActFn / MaxPoolFn, K23).  The
        # device backward is that of batch statistics: a trunk with a BatchNorm site in eval mode runs under torch autograd
        # whatever this says; one converted to SyncBatchNorm follows train_sync_bn
        train_encoder="torch",
        # read only with train_encoder = "device" when a trunk site is a train-mode SyncBatchNorm with a momentum: "torch" runs
        # such a trunk under torch autograd as a whole; "device" keeps it on K23, the BatchNorm backward split around ONE
        # all_gather of a [C, 6] float64 record per site and the ranks' sums combined in rank order (train_ops.SyncBnActFn).
        # Not one of TRAIN_SWITCHES: it selects nothing in a single process
        train_sync_bn="torch",
        # read only with train_encoder = "device": the FORWARD of the trunk's sites.  "torch" calls the stock torch operators
        # (MIOpen's convolutions, torch's batch norm and pool); "device" runs th_conv2d_fwd32 (K29: exact fp32 on the MFMA,
        # fixed-order sums), th_bn_act (K11; running statistics and num_batches_tracked updated as the module does) and
        # th_maxpool3x3s2 -- no vendor-library kernel is left in the trunk.  A SyncBatchNorm site keeps the module call for its
        # BatchNorm (the statistics span ranks); the convolutions around it follow this key.  Not one of TRAIN_SWITCHES
        train_encoder_fwd="torch",
        # patch sampling of the training targets (train_or_eval.yaml:70-75)
        patch=SimpleNamespace(use_patch_sampling=True, sample_subject_ratio=0.8, N_patches=6, size=20),
        # where the training entry's rays and patch targets come from: "batch" (as the reference: its dataset samples them on the
        # host) or "device" (made in Renderer.render from the target view, target_K / target_R / target_T and can_bounds, when the
        # batch has no ray_o; transhuman_amd/train_targets.py, K18)
        target_prep="batch",
        # which of the dataset's target sides target_prep = "device" makes: "patch" (the patch targets of a training call only) or
        # "dataset" (what the reference's __getitem__ makes for the call's split, can_smpl.py:507-535: the patch targets for a
        # training call with patch sampling, else sample_ray_h36m + get_acc -- also for the renderer's no-grad entries, which then
        # accept a batch without ray_o; transhuman_amd/train_targets.py, K26)
        target_sampler="patch",
        # sample_ray_h36m's train split (train_or_eval.yaml / lib/config/config.py: N_rand, body_sample_ratio, face_sample_ratio)
        N_rand=1024,
        body_sample_ratio=0.5,
        face_sample_ratio=0.0,
        # the trainer's loss (lib/train/trainers/if_nerf_clight.py:34-38, train_or_eval.yaml): l2rec_weight * MSE +
        # lpips_weight * mean(LPIPS_vgg) over the rendered patches (transhuman_amd/train_loss.py, K21)
        l2rec_weight=1.0,
        lpips_weight=0.1,
        # the optimiser, its schedule and the epoch loop (train_or_eval.yaml:42-43, :88-108; lib/config/config.py:53-111):
        # transhuman_amd/train_optim.py and trainer.py
        train=SimpleNamespace(optim="adam", lr=7e-4, weight_decay=0.0, epoch=3000,
                              scheduler=SimpleNamespace(type="cosine", warmup_epochs=300, decay_epochs=3000, end_lr=1e-6)),
        ep_iter=500,
        save_freq=5,
        save_latest_ep=5,
        log_interval=20,
        resume=True,
        trained_model_dir="data/trained_model",
    )


def get_cfg():
    ref = sys.modules.get("lib.config")
    if ref is not None and hasattr(ref, "cfg"):
        return ref.cfg
    return _STANDALONE


_STANDALONE = _defaults()
cfg = get_cfg()


def cfg_get(name, default=None):
    """Read a key from whichever cfg is live, falling back to our defaults."""
    c = get_cfg()
    if hasattr(c, name):
        return getattr(c, name)
    if hasattr(_STANDALONE, name):
        return getattr(_STANDALONE, name)
    return default


_ABSENT = object()


@contextmanager
def override(**values):
    """Set top-level keys of the live cfg for the length of a ``with`` block.  On exit, after an exception too, every key holds
    exactly what it held before; a key that was absent (the reference's cfg has none of the train_* keys) is deleted."""
    c = get_cfg()
    before = {k: getattr(c, k, _ABSENT) for k in values}
    try:
        for k, v in values.items():
            setattr(c, k, v)
        yield c
    finally:
        for k, v in before.items():
            if v is not _ABSENT:
                setattr(c, k, v)
            elif isinstance(c, dict):               # (a yacs node keeps its keys as dict items)
                c.pop(k, None)
            elif hasattr(c, k):
                delattr(c, k)
