"""ctypes binding of libtranshuman_hip.so (include/transhuman_hip.h).

PyTorch is used for device memory, streams and nothing else: every function
here takes CUDA(=HIP) tensors, hands raw device pointers + the current stream
to the C ABI and returns freshly allocated tensors.  There is NO fallback: if
the shared library is missing or a call fails this module raises.
"""
import ctypes as C
import os
import sys
import warnings

import torch

from . import cheader

_HERE = os.path.dirname(os.path.abspath(__file__))
# TH_LIB_PATH: developer override to A/B an experimental build of the same ABI
LIB_PATH = os.environ.get("TH_LIB_PATH") or os.path.join(_HERE, "libtranshuman_hip.so")

c_float_p = C.POINTER(C.c_float)

# The binding follows include/transhuman_hip.h (cheader.py): prototypes, struct layouts and constants are written down there
# only.  SYMBOLS: name -> (restype, [argtypes]) for every function the header declares.
_H = cheader.load()
SYMBOLS = _H.prototypes
ThLinear, ThMlpWeights, ThVitBlock, ThPoints, ThSmplModel, ThMapSource, ThFrame = (
    _H.structs[n] for n in ("th_linear", "th_mlp_weights", "th_vit_block", "th_points", "th_smpl_model", "th_map_source",
                            "th_frame"))

_lib = None


class HipError(RuntimeError):
    pass


def load_library():
    """dlopen the in-tree library and bind prototypes.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipError(f"{LIB_PATH} not found: build it with `python -m transhuman_amd.build` "
                       "(there is no CPU/torch fallback for the rendering hot path)")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    have, want = lib.th_abi_version(), _H.constants["TH_ABI_VERSION"]
    if have != want:
        raise HipError(f"{LIB_PATH} has ABI version {have}, include/transhuman_hip.h declares {want}: rebuild it with "
                       "`python -m transhuman_amd.build`")
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise HipError(_lib.th_last_error().decode())


_have_gpu = None
_NO_GPU = "no HIP device visible: the TransHuman hot path needs an MI355X (gfx950)"


def _gpu_visible():
    """torch.cuda.is_available(), asked once (it reads environment variables on every call: ~70 calls per frame showed up
    in the host profile, tools/host_cost.py)"""
    global _have_gpu
    if _have_gpu is None:
        _have_gpu = bool(torch.cuda.is_available())
    return _have_gpu


class DeviceState:
    """Everything this module keeps about ONE device; found through _state() only."""
    def __init__(self, index):
        self.index, self.handle = index, None       # (handle: the th_ctx*, created by ctx())
        # what the caller asked for through set_mlp_mode / set_vit_mode, set_tex_rows, set_fused_waves (None = never: the default)
        self.mode, self.tex_rows, self.fused_waves = {"mlp": None, "vit": None}, None, None
        # what the range guard has switched until new weights: per-layer fp32 MLP launches, stock stem convolutions, fp32 TransHE GEMMs
        self.fallback = {"mlp": False, "conv": False, "vit": False}
        self.epoch = 0                   # number of switches so far (frames queued earlier are re-rendered)
        self.owner = {}                  # "mlp" / "vit" -> (weakref to the module whose weights the ctx holds, version tuple)
        self.truncation = 0.0            # what set_truncation last handed to th_set_truncation (0: off, a new context's default)
        self.dparf = (7, 10, 0.5)        # what set_dparf last handed to th_set_dparf (cfg.KNN, KNN_FREQ, KNN_DIST_ALPHA; a new context's default)
        self.workspaces, self.pools = {}, {}   # slot -> render workspace (_cached_ws) / shading pool, None: the shared one (_shade_pool)


_states = {}      # device index -> DeviceState; a torch.device that carried an index is kept as a second key of its record


def _state(device=None):
    """The record of ``device``: None, an index, "cuda", "cuda:1" or a torch.device; without an index: the current device."""
    st = _states.get(device)             # (the per-call path: one lookup, no torch.cuda query)
    if st is None:
        index = device if isinstance(device, int) else None if device is None else torch.device(device).index
        if index is None:
            if not _gpu_visible():
                raise HipError(_NO_GPU)
            index = torch.cuda.current_device()
        st = _states.get(index) or _states.setdefault(index, DeviceState(index))
        if isinstance(device, torch.device) and device.index is not None:
            _states[device] = st
    return st


def ctx(device=None):
    st = _states.get(device)
    if st is None or st.handle is None:
        lib = load_library()
        if not _gpu_visible():
            raise HipError(_NO_GPU)
        st = _state(device)
        if st.handle is None:
            h = C.c_void_p()
            _check(lib.th_ctx_create(st.index, C.byref(h)))
            st.handle = h
    return st.handle


def _stream():
    # (torch.cuda.current_stream() builds a Stream object through three Python layers: 4-8 us, ~40 times per frame; the raw
    # handle of the current stream of the current device is one C call)
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _f32(t):
    assert t.is_cuda, "expected a device tensor"
    if t.dtype is torch.float32 and t.is_contiguous():       # (the common case: no new tensor objects)
        return t.detach() if t.requires_grad else t
    return t.detach().to(torch.float32).contiguous()


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _linear(w, b):
    w2 = _f32(w).reshape(w.shape[0], -1)
    b2 = _f32(b) if b is not None else None
    keep = (w2, b2)
    return ThLinear(_p(w2), _p(b2), w2.shape[0], w2.shape[1]), keep


# ---------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------
def set_mlp_weights(net):
    """Upload + repack the per-point MLP of a Network (cross_transformer.py:96-126)."""
    lib = load_library()
    keep = []
    W = ThMlpWeights()
    pairs = {"fc_0": net.fc_0, "alpha_res_0": net.alpha_res_0, "key0": net.spatial_key_value_0.key_embed,
             "val0": net.spatial_key_value_0.value_embed, "key1": net.spatial_key_value_1.key_embed,
             "val1": net.spatial_key_value_1.value_embed, "fc_1": net.fc_1, "fc_2": net.fc_2, "fc_3": net.fc_3,
             "alpha_fc": net.alpha_fc, "feature_fc": net.feature_fc, "rgb_res_0": net.rgb_res_0,
             "view_fc": net.view_fc, "rgb_res_1": net.rgb_res_1, "fc_4": net.fc_4, "rgb_fc": net.rgb_fc}
    # optional: the encoder's colour lift (encoder.py:95) -> colour-folded layers for the compact pixel map
    enc = getattr(net, "encoder", None)
    if enc is not None and hasattr(enc, "upsample_color"):
        pairs["upsample_color"] = enc.upsample_color
    for name, mod in pairs.items():
        lin, k = _linear(mod.weight, mod.bias)
        keep.append(k)
        setattr(W, name, lin)
    # fc_0 is 256 x (195 + 6 KNN_FREQ): the context checks it against the octave count in force, which is this network's
    dev = net.fc_0.weight.device
    st = _state(dev)
    set_dparf(st.dparf[0], net.PE_relative.num_freqs, st.dparf[2], dev)
    _check(lib.th_set_mlp_weights(ctx(dev), C.byref(W), _stream()))


def set_vit_weights(vit):
    lib = load_library()
    keep = []
    blocks = (ThVitBlock * len(vit.blocks))()
    for i, blk in enumerate(vit.blocks):
        b = blocks[i]
        for name, t in (("ln1_w", blk.norm1.weight), ("ln1_b", blk.norm1.bias), ("ln2_w", blk.norm2.weight),
                        ("ln2_b", blk.norm2.bias)):
            tt = _f32(t)
            keep.append(tt)
            setattr(b, name, tt.data_ptr())
        for name, mod in (("qkv", blk.attn.qkv), ("proj", blk.attn.proj), ("fc1", blk.mlp.fc1), ("fc2", blk.mlp.fc2)):
            lin, k = _linear(mod.weight, mod.bias)
            keep.append(k)
            setattr(b, name, lin)
    nw, nb = _f32(vit.norm.weight), _f32(vit.norm.bias)
    _check(lib.th_set_vit_weights(ctx(nw.device), len(vit.blocks), vit.embed_dim, vit.num_heads, blocks, _p(nw), _p(nb),
                                  _stream()))


_param_lists = {}      # id(module) -> [weakref(module), parameter list, calls since the last walk]


def _sync_weights(mod, kind):
    """Re-upload when the device context does not hold THIS module's current weights: a th_ctx has one MLP and
    one ViT weight image per device, so ownership is tracked per device and kind -- rendering with net A, then
    net B, then A again re-uploads A (a cache keyed by id(module) alone would find A's old version tuple and
    shade A with B's weights; the same for a new module that lands on a freed module's id()).  Any parameter
    change (load_state_dict, .cuda(), optimiser step) bumps the version tuple.
    The check runs every frame, so it is kept cheap: the module tree is walked once (and again every 256 calls,
    in case a Parameter object was replaced), per call only the in-place version counters of the cached
    parameter list and the addresses of its first / last tensor are read (25 us instead of 0.9 ms for the
    310-tensor Network: the walk used to leave the GPU idle in front of the per-sample stage)."""
    import weakref
    if not _gpu_visible():
        raise HipError(_NO_GPU + "; there is no CPU fallback")
    ent = _param_lists.get(id(mod))
    if ent is None or ent[0]() is not mod or ent[2] >= 256:
        ent = [weakref.ref(mod), list(mod.parameters()), 0]
        _param_lists[id(mod)] = ent
        if len(_param_lists) > 64:                       # drop entries of modules that are gone
            for k in [k for k, v in _param_lists.items() if v[0]() is None]:
                del _param_lists[k]
    ent[2] += 1
    pl = ent[1]
    ver = (tuple(p._version for p in pl), pl[0].data_ptr(), pl[-1].data_ptr(), len(pl))
    dev = pl[0].device
    st = _state(dev)
    own = st.owner.get(kind)
    if own is None or own[0]() is not mod or own[1] != ver:
        # The context's packed weight image is rewritten in place on the CURRENT stream.  Frame pipelines call this from a
        # side stream while kernels of earlier frames may still read the image on the shading stream (and the other way
        # round): a weight change is rare (load_state_dict, an optimiser step between evaluations), so it simply drains the
        # device first.
        if own is not None:
            torch.cuda.synchronize(dev)
        (set_mlp_weights if kind == "mlp" else set_vit_weights)(mod)
        st.owner[kind] = (weakref.ref(mod), ver)
        if kind == "vit":
            _vit_graph_epoch[0] += 1
        # new weights: back to the modes the caller asked for (the guard re-checks them).  The Network's parameter set
        # includes the encoder, so the stem convolutions return to the HIP kernels with it (th_set_mlp_weights clears
        # their sticky range slot, th_set_vit_weights TransHE's).
        _restore(st, kind)
        if kind == "mlp":
            _restore(st, "conv")


# ---------------------------------------------------------------------------
# range guard of the fp16 hi/lo split arithmetic (include/transhuman_hip.h: th_range_*)
# ---------------------------------------------------------------------------
RANGE_NAMES = ("f", "s", "p", "n", "inter", "fc4_in", "conv_in", "vit_in")
RANGE_FP16_LIMIT = _H.constants["TH_RANGE_FP16_LIMIT"]     # 6.0e4 as an fp16 bit pattern (inf / NaN are larger)
RANGE_FP16_FLOOR = _H.constants["TH_RANGE_FP16_FLOOR"]     # 2^-6
RANGE_FP32_LIMIT = 0x476A6000      # 6.0e4 as an fp32 bit pattern (slot conv_in)
last_range = None                  # the last table read (debugging / tests)


def conv_fallback(device=None):
    """True while the stem convolutions of this device run through the stock modules (range guard)."""
    return _state(device).fallback["conv"]


def vit_fallback(device=None):
    """True while TransHE's dense layers of this device run on the fp32 MFMA GEMMs (range guard)."""
    return _state(device).fallback["vit"]


def guard_state(device=None):
    """What the range guard has switched on this device: every entry False = the fast paths are in use (a tripped MLP
    guard means per-layer fp32 MFMA launches, ~7x slower frames)."""
    st = _state(device)
    return {"mlp_fp32_fallback": st.fallback["mlp"], "conv_fallback": st.fallback["conv"],
            "vit_fp32_fallback": st.fallback["vit"], "epoch": st.epoch}


def range_epoch(device=None):
    return _state(device).epoch


def range_read(slot, device=None):
    """The launch-wide maxima of snapshot ``slot`` (th_range_read; waits for the work in front of the snapshot).
    None when the snapshot has been overwritten by later ones (the ring holds the 8 most recent)."""
    global last_range
    out = (C.c_uint32 * 8)()
    rc = load_library().th_range_read(ctx(device), int(slot), out)
    if rc == 2:
        return None
    _check(rc)
    last_range = list(out)
    return last_range


def range_verdict(vals):
    """-> None when every split tensor stayed inside the range the fp16 hi/lo arithmetic resolves, else a text."""
    bad = []
    for i in range(6):
        v = vals[i]
        if v >= RANGE_FP16_LIMIT:
            bad.append(f"{RANGE_NAMES[i]}: |x| reached the fp16 limit (bits 0x{v:04x})")
        elif 0 < v < RANGE_FP16_FLOOR:
            bad.append(f"{RANGE_NAMES[i]}: max |x| below 2^-6 (bits 0x{v:04x})")
    return "; ".join(bad) if bad else None


def range_trips(vals, fallback):
    """The switches the range table ``vals`` (8 words) trips on a device whose switches stand as ``fallback`` says, one that is
    set already left out: [(kind, text of the warning)] in the order the warnings appear.  No library call, no torch call."""
    trips = []
    if vals[7] >= RANGE_FP16_LIMIT and not fallback["vit"]:
        trips.append(("vit", "an operand of TransHE's dense layers left the fp16 range; using the fp32 MFMA GEMMs until new "
                             "weights are uploaded"))
    if vals[6] >= RANGE_FP32_LIMIT and not fallback["conv"]:
        trips.append(("conv", "the ResNet-stem convolution input left the fp16 range; using the stock convolutions until new "
                              "weights are uploaded"))
    why = range_verdict(vals)
    if why is not None and not fallback["mlp"]:
        trips.append(("mlp", "activations left the range of the fp16 hi/lo split MFMA kernel (" + why + "); re-rendering and "
                             "continuing on the per-layer fp32 MFMA path for these weights"))
    return trips


def _set_mode(st, kind, mode):
    _check(getattr(load_library(), "th_set_%s_mode" % kind)(ctx(st.index), mode))
    if kind == "vit":
        _vit_graph_epoch[0] += 1         # (captured TransHE graphs hold the other arithmetic)


def _trip(st, kind, text):
    """The one place a switch is set ("conv" has no mode in the library: conv2d_supported asks the flag)."""
    warnings.warn("transhuman_amd: " + text, RuntimeWarning)
    if kind != "conv":
        _set_mode(st, kind, 0)
    st.fallback[kind] = True
    st.epoch += 1


def _restore(st, kind, mode=None):
    """The one place a switch is cleared.  ``mode`` None: new weights, a tripped switch goes back to the mode the caller asked for.
    Else the caller asks for ``mode`` now; TransHE's fp32 form leaves a tripped switch standing (its slot is sticky)."""
    if mode is not None:
        _set_mode(st, kind, mode)
        st.mode[kind] = mode
        if kind == "vit" and mode == 0:
            return
    elif st.fallback[kind] and kind != "conv":
        _set_mode(st, kind, 1 if st.mode[kind] is None else st.mode[kind])
    st.fallback[kind] = False


def force_conv_fallback(device, why):
    """Switch the stem convolutions of this device to the stock modules (what the range guard does when slot conv_in trips)
    on evidence from outside the context's own range table -- e.g. non-finite stem latents received from another rank
    (dist.StemExchange).  Bumps the epoch: frames built before are rebuilt."""
    st = _state(device)
    if not st.fallback["conv"]:
        _trip(st, "conv", why + "; using the stock convolutions until new weights are uploaded")


def _guard(device, slot):
    """True when the snapshot is clean.  Otherwise the context has been switched to the fp32 path (and / or the
    stem convolutions to the stock modules, TransHE to the fp32 GEMMs): the caller re-runs its work.  Every switch
    bumps the device's epoch: the conv / TransHE slots are sticky and written by the stream that computes the NEXT
    frames' constants, so an overflow of frame j+1 usually shows up in the snapshot of frame j -- frames whose
    constants were built before the switch are recognised by their older epoch and rebuilt (render_sequence)."""
    if slot is None or slot < 0:
        return True
    vals = range_read(slot, device)
    if vals is None:             # overwritten snapshot: the frame is unchecked -> render it again (its own snapshot is read at once)
        return False
    st = _state(device)
    trips = range_trips(vals, st.fallback)
    for kind, text in trips:
        _trip(st, kind, text)
    return not trips


def _guarded(device, launch, launches, frame=None, check_last=True):
    """``launch(frame, i)`` queues try ``i`` and returns its snapshot id.  A snapshot that is not clean (or was overwritten before
    it could be read) means the paths the guard switched are in effect now: the frame's constants are built again if the stem or
    TransHE was switched, and the next try's snapshot is checked too -- bounded by ``launches``: every switch is one-way, three
    cover MLP + stem + TransHE tripping one after the other.  ``check_last`` False: the last try's snapshot is left unread."""
    for i in range(launches):
        slot = launch(frame, i)
        if (i + 1 == launches and not check_last) or _guard(device, slot):
            break
        if frame is not None and frame.rebuild is not None and (conv_fallback(device) or vit_fallback(device)):
            frame = frame.rebuild()


# ---------------------------------------------------------------------------
# building blocks (used by tests and by the Network/Renderer classes)
# ---------------------------------------------------------------------------
def linear(x, weight, bias=None, act=0):
    """C = act(x @ W^T + b) on the fp32 MFMA pipe.  x [M,K] (row stride % 4 == 0)."""
    lib = load_library()
    x = _f32(x)
    assert x.dim() == 2
    if x.shape[1] % 4:
        x = torch.nn.functional.pad(x, (0, 4 - x.shape[1] % 4))
    lin, keep = _linear(weight, bias)
    out = torch.empty((x.shape[0], lin.out_f), dtype=torch.float32, device=x.device)
    ws = _ws(lib.th_linear_workspace_bytes(lin.out_f, lin.in_f), x.device)
    _check(lib.th_linear_forward(ctx(x.device), _p(x), x.stride(0), x.shape[0], C.byref(lin), act, _p(out),
                                 out.stride(0), _p(ws), ws.numel(), _stream()))
    return out


class Points:
    """Host-side holder of a th_points (keeps the tensors alive)."""

    def __init__(self, ray_o=None, ray_d=None, near=None, far=None, n_samples=1, pts=None, z_vals=None, sigma_noise=None):
        """``z_vals`` [R,S]: explicit sample depths (the reference's stratified jitter, if_clight_renderer.py:276-283) instead of
        near (1 - t) + far t; ``sigma_noise`` [R,S]: added to sigma in front of raw2alpha's relu (nerf_net_utils.py:39-44)."""
        # a pending render_prepass of these rays: (verts, workspace) it ran in and its cluster count (render_prepass), whether the
        # producers of its first chunks have been queued (render_pregather); render_rays consumes all four
        self._prepass_pending, self._prepass_keep, self._prepass_nc, self._pregathered = False, None, 0, False
        if pts is not None:
            self.pts = _f32(pts).reshape(-1, 3)
            self.R, self.S = self.pts.shape[0], 1
            self.keep = (self.pts,)
            self.c = ThPoints(_p(self.pts), None, None, None, None, None, None, self.R, 1)
            return
        self.ray_o, self.ray_d = _f32(ray_o).reshape(-1, 3), _f32(ray_d).reshape(-1, 3)
        self.near, self.far = _f32(near).reshape(-1), _f32(far).reshape(-1)
        dev = self.ray_o.device
        # t_vals exactly as torch.linspace builds them (if_clight_renderer.py:273-274); cached per (S, device)
        self.t, self.omt = _t_vals(n_samples, dev)
        self.R, self.S = self.ray_o.shape[0], n_samples
        self.z_vals = None if z_vals is None else _f32(z_vals).reshape(self.R, self.S)
        self.sigma_noise = None if sigma_noise is None else _f32(sigma_noise).reshape(self.R, self.S)
        self.c = ThPoints(None, _p(self.ray_o), _p(self.ray_d), _p(self.near), _p(self.far), _p(self.t), _p(self.omt),
                          self.R, self.S, _p(self.z_vals), _p(self.sigma_noise))


_t_cache = {}


def _t_vals(n_samples, dev):
    key = (int(n_samples), str(dev))
    if key not in _t_cache:
        t = torch.linspace(0.0, 1.0, steps=n_samples)
        _t_cache[key] = (t.to(dev), (1.0 - t).to(dev))
    return _t_cache[key]


def hull_mask(points, verts_world, thresh=0.1):
    lib = load_library()
    v = _f32(verts_world).reshape(-1, 3)
    P = points.R * points.S
    mask = torch.empty(P, dtype=torch.uint8, device=v.device)
    hit = torch.empty(points.R, dtype=torch.int32, device=v.device)
    ws = _ws(lib.th_hull_workspace_bytes(v.shape[0]), v.device)
    _check(lib.th_hull_mask(ctx(v.device), C.byref(points.c), _p(v), v.shape[0], thresh, _p(mask), _p(hit), _p(ws),
                            ws.numel(), _stream()))
    return mask.view(points.R, points.S).bool(), hit.bool()


def pack_cams(R, T, K):
    """[V,3,3],[V,3,1],[V,3,3] -> [V,21] fp32 (R | T | K row-major)."""
    V = R.shape[0]
    return torch.cat([_f32(R).reshape(V, 9), _f32(T).reshape(V, 3), _f32(K).reshape(V, 9)], dim=1).contiguous()


def feat_scale(scale_np, image_shape, device):
    """sample_from_feature_map, if_clight_renderer.py:193-195 (float64 divide, cast to fp32)."""
    import numpy as np
    s = np.asarray(scale_np, dtype=np.float64) / np.asarray(image_shape, dtype=np.float64)
    key = (float(s[0]), float(s[1]), str(device))
    if key not in _scale_cache:
        _scale_cache[key] = torch.tensor(s).to(dtype=torch.float32, device=device)
    return _scale_cache[key]


_scale_cache = {}


def csr_to_device(offsets, members, device):
    return (torch.as_tensor(offsets, dtype=torch.int32, device=device).contiguous(),
            torch.as_tensor(members, dtype=torch.int32, device=device).contiguous())


def paint_group(holder_map, verts_world, cams, scale_xy, vizmap, off, mem, return_painted=False):
    lib = load_library()
    m = _f32(holder_map)
    V, Cc, H, W = m.shape
    v = _f32(verts_world).reshape(-1, 3)
    nc = off.numel() - 1
    viz = vizmap.to(torch.uint8).contiguous() if vizmap is not None else None
    painted = torch.empty((V, v.shape[0], Cc), dtype=torch.float32, device=m.device)
    tokens = torch.empty((V, nc, Cc), dtype=torch.float32, device=m.device)
    _check(lib.th_paint_group(ctx(m.device), _p(m), V, Cc, H, W, _p(v), v.shape[0], _p(cams), _p(scale_xy), _p(viz),
                              _p(off), _p(mem), nc, _p(painted), _p(tokens), _stream()))
    return (tokens, painted) if return_painted else tokens


class SplitMap:
    """The compact pixel map in the TH_MAP_SPLIT layout: one buffer holding [V,H,W,256] latents (1 KiB rows: a corner
    texel is ONE aligned wave load; the interleaved 260-channel rows straddle nine 128-byte lines instead of eight and
    cost a second load instruction for their 65th float4) followed by [V,H,W,4] (r, g, b, 0)."""

    def __init__(self, buf, V, H, W, source=None):
        self.buf, self.V, self.H, self.W = buf, V, H, W
        self.shape = (V, H, W, 256)
        self.device = buf.device
        # cropped map (upsample_concat_split(box=...)): (ThMapSource, the tensors it points to); texels outside the
        # per-view box are NOT written until a frame-level call needs them (th_frame.map_source)
        self.source = source
        # th_map_fold's output for this map ([2, V, H, W, 256] fp32; hip.map_fold), or None: frames built on the map then take
        # the texel hand-over (th_frame.map_fold)
        self.fold = None

    @property
    def box(self):
        """device int32 [V,4] (x0, y0, x1, y1 inclusive) of a cropped map, else None"""
        return self.source[1][0] if self.source is not None else None

    @property
    def demand(self):
        """the render_predemand buffer a demand-driven map was written for, else None"""
        return self.source[1][5] if self.source is not None and len(self.source[1]) > 5 else None

    def data_ptr(self):
        return self.buf.data_ptr()

    @property
    def latents(self):
        return self.buf[: self.V * self.H * self.W * 256].view(self.V, self.H, self.W, 256)

    @property
    def rgb0(self):
        return self.buf[self.V * self.H * self.W * 256:].view(self.V, self.H, self.W, 4)

    def interleaved(self):
        """the same map as one [V,H,W,260] tensor (tests / A-B)"""
        return torch.cat([self.latents, self.rgb0], dim=-1).contiguous()


def map_fold(net, split_map):
    """th_map_fold: alpha_res_0 / rgb_res_0 (under the folded view_fc) / rgb_res_1 of ``net`` applied to the texels of
    ``split_map`` (inside its crop box), on the current stream; the result is kept as ``split_map.fold``."""
    assert isinstance(split_map, SplitMap)
    _sync_weights(net, "mlp")
    V, H, W = split_map.V, split_map.H, split_map.W
    fold = torch.empty((2, V, H, W, 256), dtype=torch.float32, device=split_map.device)
    if split_map.demand is not None:          # demand-driven map: the texels the frame's samples read, as a compacted list
        _check(load_library().th_map_fold_demand(ctx(split_map.device), _p(split_map), V, H, W, _p(split_map.demand), _p(fold), _stream()))
        split_map.fold = fold
        return fold
    if split_map.box is not None:
        _box_checked(split_map.box, H)
    _check(load_library().th_map_fold(ctx(split_map.device), _p(split_map), V, H, W, _p(split_map.box), _p(fold), _stream()))
    split_map.fold = fold
    return fold


def map_box(verts_a, verts_b, cams, scale_xy, H, W, reach):
    """th_map_box: per view the texel box (device int32 [V,4]: x0, y0, x1, y1 inclusive) that holds every texel a
    bilinear gather at a point within ``reach`` (per axis) of a vertex of verts_a / verts_b can read."""
    lib = load_library()
    a = _f32(verts_a).reshape(-1, 3)
    b = _f32(verts_b).reshape(-1, 3) if verts_b is not None else None
    V = cams.shape[0]
    # [V,4] boxes followed by [V,H,2] row spans (x0, x1 of every image row: the outline of the body inside the box); the
    # returned tensor is the [V,4] head of that buffer, `map_spans(box, H)` views the rest
    buf = torch.empty(V * 4 + V * int(H) * 2 + V, dtype=torch.int32, device=a.device)      # (+ V flag words of the kernels)
    box = buf[: V * 4].view(V, 4)
    box._th_map_box = (buf, int(H))              # (a clone / an exchanged [V,4] copy has no spans behind it: _box_checked)
    _check(lib.th_map_box(ctx(a.device), _p(a), a.shape[0], _p(b), b.shape[0] if b is not None else 0, _p(cams), V,
                          _p(scale_xy), int(H), int(W), float(reach), _p(box), _stream()))
    return box


def _box_checked(box, H):
    """``box`` must be the tensor hip.map_box returned (the row spans and flag words th_map_box wrote sit BEHIND it in the
    same buffer and the C side reads them through the box pointer): a copy of the [V,4] values is refused"""
    tag = getattr(box, "_th_map_box", None)
    if tag is None or tag[0].data_ptr() != box.data_ptr() or tag[1] != int(H):
        raise HipError("box must be the tensor hip.map_box returned for this image height (its row spans follow it in memory)")
    return box


def map_spans(box, H):
    """the [V,H,2] row spans (x0, x1 inclusive; x1 < x0: empty row) th_map_box wrote behind the boxes of ``box``"""
    _box_checked(box, H)
    V = box.shape[0]
    return torch.as_strided(box, (V, int(H), 2), (int(H) * 2, 2, 1), storage_offset=box.storage_offset() + V * 4)


def upsample_concat_split(images, lat0, lat1, lat2, box=None, reach=0.0, demand=None):
    """th_upsample_concat_split(_box): the compact map (colour lift folded into the consumers) in the split layout.
    ``box`` (map_box, computed with ``reach``): only the texels of each view's box are written -- the returned SplitMap
    carries what it was made from (``source``) and hip.Frame hands that to the C side, which completes the map on its
    own if a call gathers outside the hull's reach (un-masked small-frame branch, no hull test)."""
    lib = load_library()
    img, l0, l1, l2 = _f32(images), _f32(lat0), _f32(lat1), _f32(lat2)
    V, _, H, W = img.shape
    assert l0.shape[1] == 64 and l1.shape[1] == 64 and l2.shape[1] == 128
    dims = (C.c_int32 * 6)(l0.shape[2], l0.shape[3], l1.shape[2], l1.shape[3], l2.shape[2], l2.shape[3])
    buf = torch.empty(V * H * W * 260, dtype=torch.float32, device=img.device)
    if demand is not None:
        # demand-driven map (render_predemand): only the texels the frame's valid samples / painted vertices read are written
        _check(lib.th_upsample_concat_split_demand(ctx(img.device), _p(img), _p(l0), _p(l1), _p(l2), dims, V, H, W, _p(buf), None,
                                                   _p(demand), _stream()))
        src = ThMapSource(None, float(reach), _p(img), _p(l0), _p(l1), _p(l2), dims, _p(demand))
        return SplitMap(buf, V, H, W, source=(src, (None, img, l0, l1, l2, demand)))
    if box is None:
        _check(lib.th_upsample_concat_split(ctx(img.device), _p(img), _p(l0), _p(l1), _p(l2), dims, V, H, W, _p(buf), _stream()))
        return SplitMap(buf, V, H, W)
    assert box.dtype == torch.int32 and tuple(box.shape) == (V, 4) and box.is_contiguous()
    # (th_map_box's buffer: the row spans follow the boxes)
    _box_checked(box, H)
    _check(lib.th_upsample_concat_split_box(ctx(img.device), _p(img), _p(l0), _p(l1), _p(l2), dims, V, H, W, _p(buf),
                                            _p(box), _stream()))
    src = ThMapSource(_p(box), float(reach), _p(img), _p(l0), _p(l1), _p(l2), dims, None)
    return SplitMap(buf, V, H, W, source=(src, (box, img, l0, l1, l2)))


def upsample_concat_nhwc(images, lat0, lat1, lat2, color_w=None, color_b=None):
    """Encoder tail (encoder.py:133-146) -> channels-last pixel_feat_map [V,H,W,384], or with
    color_w=None the compact map [V,H,W,260] (256 latent | r g b | 0; the lift is folded into the consumers)."""
    lib = load_library()
    img, l0, l1, l2 = _f32(images), _f32(lat0), _f32(lat1), _f32(lat2)
    V, _, H, W = img.shape
    assert l0.shape[1] == 64 and l1.shape[1] == 64 and l2.shape[1] == 128
    dims = (C.c_int32 * 6)(l0.shape[2], l0.shape[3], l1.shape[2], l1.shape[3], l2.shape[2], l2.shape[3])
    cw = _f32(color_w).reshape(128, 3) if color_w is not None else None
    cb = _f32(color_b) if color_w is not None else None
    out = torch.empty((V, H, W, 384 if color_w is not None else 260), dtype=torch.float32, device=img.device)
    _check(lib.th_upsample_concat_nhwc(ctx(img.device), _p(img), _p(l0), _p(l1), _p(l2), dims, V, H, W, _p(cw), _p(cb),
                                       _p(out), _stream()))
    return out


def paint_group_nhwc(map_nhwc, verts_world, cams, scale_xy, vizmap, red_w, red_b, off, mem, color_w=None,
                     color_b=None):
    """Sample the channels-last map at the projected vertices, apply reduction_layer there, mask, pool.
    A compact (260-channel) map needs the colour lift (color_w, color_b) to fold into the reduction layer."""
    lib = load_library()
    V, H, W, Cc = map_nhwc.shape                      # (a SplitMap reports 256 channels: TH_MAP_SPLIT)
    v = _f32(verts_world).reshape(-1, 3)
    nc = off.numel() - 1
    viz = vizmap.to(torch.uint8).contiguous() if vizmap is not None else None
    lin, keep = _linear(red_w, red_b)
    lift, keep2 = _linear(color_w, color_b) if color_w is not None else (None, None)
    tokens = torch.empty((V, nc, lin.out_f), dtype=torch.float32, device=v.device)
    ws = _ws(lib.th_paint_group_nhwc_workspace_bytes(V, v.shape[0], Cc, lin.out_f), v.device)
    _check(lib.th_paint_group_nhwc(ctx(v.device), _p(map_nhwc), V, H, W, Cc, _p(v), v.shape[0], _p(cams), _p(scale_xy),
                                   _p(viz), C.byref(lin), C.byref(lift) if lift is not None else None, _p(off), _p(mem),
                                   nc, _p(tokens), _p(ws), ws.numel(), _stream()))
    return tokens


_conv_cache = {}


def conv2d_supported(conv):
    """True for the nn.Conv2d shapes th_conv2d is built for (the bias-free convolutions of the ResNet18 stem)."""
    ks, st, pd = conv.kernel_size, conv.stride, conv.padding
    return (not conv_fallback(conv.weight.device) and conv.bias is None and ks[0] == ks[1] and st[0] == st[1] and pd[0] == pd[1] == ks[0] // 2 and
            conv.groups == 1 and conv.dilation == (1, 1) and
            bool(load_library().th_conv2d_supported(conv.in_channels, conv.out_channels, ks[0], st[0])))


def conv2d(x, conv, stats=False):
    """th_conv2d: y = conv(x) for a supported bias-free nn.Conv2d (NCHW fp32), fp16-split MFMA implicit GEMM.
    The packed weight image is cached per module and rebuilt when the weight tensor changes.
    ``stats=True`` (th_conv2d_stats): also returns the per-channel BatchNorm partial sums the epilogue leaves, as
    (y, (buffer, n_partials)) for bn_act(..., conv_stats=...)."""
    lib = load_library()
    assert x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous()
    w = conv.weight
    key = id(conv)
    ent = _conv_cache.get(key)
    if ent is None or ent[0] is not w or ent[1] != w._version or ent[2].device != x.device:
        co, ci, ks, _ = w.shape
        buf = torch.empty(lib.th_conv_pack_bytes(co, ci, ks), dtype=torch.uint8, device=x.device)
        inv = C.c_float()
        _check(lib.th_conv_pack(ctx(x.device), _p(_f32(w)), co, ci, ks, _p(buf), buf.numel(), C.byref(inv), _stream()))
        ent = (w, w._version, buf, float(inv.value))
        _conv_cache[key] = ent
    N, ci, H, W = x.shape
    co, ks, st = conv.out_channels, conv.kernel_size[0], conv.stride[0]
    pd = ks // 2
    Ho, Wo = (H + 2 * pd - ks) // st + 1, (W + 2 * pd - ks) // st + 1
    y = torch.empty((N, co, Ho, Wo), dtype=torch.float32, device=x.device)
    if stats:
        npart = int(lib.th_conv2d_stats_partials(N, ci, H, W, co, ks, st))
        sbuf = torch.empty((co, npart, 2), dtype=torch.float32, device=x.device)
        _check(lib.th_conv2d_stats(ctx(x.device), _p(x), N, ci, H, W, _p(ent[2]), ent[3], co, ks, st, _p(y), _p(sbuf),
                                   sbuf.numel() * 4, _stream()))
        return y, (sbuf, npart)
    _check(lib.th_conv2d(ctx(x.device), _p(x), N, ci, H, W, _p(ent[2]), ent[3], co, ks, st, _p(y), _stream()))
    return y


def maxpool3x3s2(x):
    """th_maxpool3x3s2: nn.MaxPool2d(3, 2, 1) on NCHW fp32."""
    assert x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous()
    N, Cc, H, W = x.shape
    y = torch.empty((N, Cc, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device)
    _check(load_library().th_maxpool3x3s2(ctx(x.device), _p(x), N * Cc, H, W, _p(y), _stream()))
    return y


def bn_act(x, bn, residual=None, relu=True, conv_stats=None):
    """th_bn_act: train-mode nn.BatchNorm2d `bn` on x [N,C,H,W] (+ residual) (+ ReLU) in two launches; updates
    bn.running_mean / running_var like the module (num_batches_tracked is left to the caller).  A module in eval() mode
    normalises with its running statistics in one launch (th_bn_act_eval).  ``conv_stats`` = the (buffer, n_partials) of
    conv2d(..., stats=True) that produced x: the statistics pass is skipped (th_bn_act_stats, one launch)."""
    lib = load_library()
    assert x.dim() == 4 and x.is_contiguous() and x.dtype == torch.float32
    N, Cc, H, W = x.shape
    r = None if residual is None else residual.contiguous()
    if not bn.training:             # eval(): running statistics, one launch (th_bn_act_eval)
        assert bn.track_running_stats and bn.running_mean is not None, "eval-mode BatchNorm without running statistics"
        y = torch.empty_like(x)
        _check(lib.th_bn_act_eval(ctx(x.device), _p(x), None if r is None else _p(r), N, Cc, H * W,
                                  None if bn.weight is None else _p(bn.weight), None if bn.bias is None else _p(bn.bias),
                                  float(bn.eps), _p(bn.running_mean), _p(bn.running_var), int(relu), _p(y), _stream()))
        return y
    y = torch.empty_like(x)
    track = bn.track_running_stats and bn.running_mean is not None
    assert bn.momentum is not None, "cumulative-average BatchNorm (momentum=None) is not handled here"
    mom = float(bn.momentum)
    r = None if residual is None else residual.contiguous()
    if conv_stats is not None:
        sbuf, npart = conv_stats
        assert sbuf.shape == (Cc, npart, 2) and sbuf.dtype == torch.float32 and sbuf.device == x.device
        _check(lib.th_bn_act_stats(ctx(x.device), _p(x), None if r is None else _p(r), N, Cc, H * W, _p(sbuf), npart,
                                   None if bn.weight is None else _p(bn.weight), None if bn.bias is None else _p(bn.bias),
                                   float(bn.eps), mom, _p(bn.running_mean) if track else None,
                                   _p(bn.running_var) if track else None, int(relu), _p(y), _stream()))
        return y
    ws = _ws(lib.th_bn_workspace_bytes(N, Cc, H * W), x.device)
    _check(lib.th_bn_act(ctx(x.device), _p(x), None if r is None else _p(r), N, Cc, H * W,
                         None if bn.weight is None else _p(bn.weight), None if bn.bias is None else _p(bn.bias),
                         float(bn.eps), mom, _p(bn.running_mean) if track else None,
                         _p(bn.running_var) if track else None, int(relu), _p(y), _p(ws), ws.numel(), _stream()))
    return y


def segment_mean(src, off, mem):
    lib = load_library()
    s = _f32(src)
    width = int(s[0].numel())
    s2 = s.reshape(s.shape[0], width)
    nc = off.numel() - 1
    out = torch.empty((nc, width), dtype=torch.float32, device=s.device)
    _check(lib.th_segment_mean_f32(ctx(s.device), _p(s2), width, _p(off), _p(mem), nc, _p(out), _stream()))
    return out.reshape(nc, *s.shape[1:])


def segment_mean_rot(blend, off, mem):
    """blend [n_verts,4,4] (float64 kept as is) -> fp32 [N_c,3,3]."""
    lib = load_library()
    b = blend.detach().to(torch.float64).contiguous().reshape(-1, 16)
    nc = off.numel() - 1
    out = torch.empty((nc, 9), dtype=torch.float32, device=b.device)
    _check(lib.th_segment_mean_rot_f64(ctx(b.device), _p(b), _p(off), _p(mem), nc, _p(out), _stream()))
    return out


_graphs_off = [False]


def graph_capture(fn):
    """Record the launches ``fn()`` queues on the current stream into a hipGraph (torch.cuda.CUDAGraph, private memory pool)
    -> (graph, fn's result).  Capture mode "thread_local": API calls other threads make meanwhile (the process group's
    watchdog polling its events in a multi-rank job) neither fail nor invalidate the capture.  A capture that fails raises
    GraphCaptureFailed after switching the replayed-graph forms off for the process (callers run their eager form)."""
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            out = fn()
    except Exception as e:           # (nothing of fn ran; the capture is over either way)
        _graphs_off[0] = True
        import warnings
        warnings.warn(f"transhuman_amd: hipGraph capture failed ({type(e).__name__}: {e}); the stem and TransHE run as "
                      "separate launches from here on", RuntimeWarning)
        raise GraphCaptureFailed(str(e)) from e
    return g, out


class GraphCaptureFailed(RuntimeError):
    pass


def graphs_enabled():
    return not _graphs_off[0]


_vit_graphs = {}
def graph_epoch():
    """counter bumped whenever captured graphs are dropped for new weights / arithmetic (frame pipelines key their priming on it)"""
    return _vit_graph_epoch[0]


_vit_graph_epoch = [0]      # bumped whenever the context's TransHE weights or arithmetic change: captured graphs are dropped
VIT_GRAPH_RING = 4


def _vit_forward_graphed(vit, x, pe):
    """TransHE's 63 launches replayed as one hipGraph (the frame paths: Renderer.render_fast / render_sequence).  Per (module,
    shape, device): the first call of a version runs eagerly and captures VIT_GRAPH_RING instances (static input copy + output
    in the graph's private pool), later calls copy the input into the next instance and replay it.  The tokens returned stay valid
    until VIT_GRAPH_RING - 1 further graphed calls of the shape have been made (the frame pipeline holds three frames).
    The captured forward holds kernel nodes only (k_vit.hip: zero16_kernel, profiles/r05_l_vit_graph_memset_node.txt).
    None = not applicable (TH_VIT_GRAPH=0, autograd input)."""
    if os.environ.get("TH_VIT_GRAPH", "1") == "0" or _graphs_off[0] or (torch.is_grad_enabled() and x.requires_grad):
        return None
    key = (id(vit), tuple(x.shape), str(x.device))
    ver = (_vit_graph_epoch[0], pe.data_ptr(), _state(x.device).owner.get("vit", (None, None))[1])
    st = _vit_graphs.get(key)
    if st is not None and st.get("eager_only"):
        st["same"] = st["same"] + 1 if st["ver"] == ver else 0          # (a version that has settled gets its graphs back)
        st["ver"] = ver
        if st["same"] < 2:
            return None
        st = None
    if st is None or st["ver"] != ver:
        # first call of a version: eagerly (the kernels' first launches must not happen under capture), then every instance of
        # the ring is captured at once -- the cost of capturing (a device synchronisation each) lands in this one call, not in
        # the next VIT_GRAPH_RING frames of a stream (a rank of N computes TransHE every N-th frame only)
        # (a version that changes with every call -- weights updated between frames, a positional table converted anew each time --
        # would capture on every call: after three captures that were never replayed the module stays on separate launches)
        thrash = 0 if st is None or st["replays"] > 0 else st["thrash"] + 1
        if thrash >= 3:
            _vit_graphs[key] = {"eager_only": True, "mod": vit, "ver": ver, "same": 0}
            return None
        if len(_vit_graphs) > 8:
            _vit_graphs.clear()
        st = _vit_graphs[key] = {"ver": ver, "inst": [], "next": 0, "mod": vit, "pe": pe,     # (the graphs hold pe's address)
                                 "replays": 0, "thrash": thrash}
        out = vit_forward(vit, x, pe, graph=False, _checked=True)
        try:
            for _ in range(VIT_GRAPH_RING):
                xs = torch.empty_like(x)
                g, o = graph_capture(lambda: vit_forward(vit, xs, pe, graph=False, _checked=True))
                st["inst"].append((g, xs, o))
        except GraphCaptureFailed:
            _vit_graphs.pop(key, None)
        return out
    k = st["next"]
    st["next"] = (k + 1) % VIT_GRAPH_RING
    st["replays"] += 1
    g, xs, out = st["inst"][k]
    xs.copy_(x)
    g.replay()
    return out


def vit_forward(vit, x, pe, graph=False, _checked=False):
    lib = load_library()
    if not _checked:
        _sync_weights(vit, "vit")
    x, pe = _f32(x), _f32(pe)
    if graph:
        out = _vit_forward_graphed(vit, x, pe)
        if out is not None:
            return out
    V, N, D = x.shape
    out = torch.empty_like(x)
    ws = _ws(lib.th_vit_workspace_bytes(V, N, D, vit.num_heads), x.device)
    _check(lib.th_vit_forward(ctx(x.device), _p(x), _p(pe), V, N, _p(out), _p(ws), ws.numel(), _stream()))
    return out


def attention(qkv, heads=3, form=0):
    """th_attention: one TransHE layer's softmax(q k^T / 8) v on its own.  qkv [V, N, 3 * heads * 64] as the qkv layer
    writes it -> [V, N, heads * 64].  form 0: the kernel the forward picks at this N; 2 / 3: attn2_kernel / attn3_kernel."""
    lib = load_library()
    qkv = _f32(qkv)
    V, N, C3 = qkv.shape
    if C3 != 3 * heads * 64:
        raise ValueError(f"qkv has {C3} columns, {heads} heads of 64 need {3 * heads * 64}")
    out = torch.empty((V, N, heads * 64), dtype=torch.float32, device=qkv.device)
    ws = _ws(lib.th_attention_workspace_bytes(V, N, heads), qkv.device)
    _check(lib.th_attention(ctx(qkv.device), _p(qkv), V, N, heads, int(form), _p(out), _p(ws), ws.numel(), _stream()))
    return out


def _attn_dims(qkv, heads):
    V, N, C3 = qkv.shape
    if C3 != 3 * heads * 64:
        raise ValueError(f"qkv has {C3} columns, {heads} heads of 64 need {3 * heads * 64}")
    return V, N


def attention_train(qkv, heads=3, form=0):
    """th_attention_train: attention() (the same kernels, the same bits) that also returns each row's log-sum-exp of the
    scaled logits -> (out [V, N, heads * 64], lse [V, heads, N]); what attention_bwd needs beside qkv."""
    lib = load_library()
    qkv = _f32(qkv)
    V, N = _attn_dims(qkv, heads)
    out = torch.empty((V, N, heads * 64), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((V, heads, N), dtype=torch.float32, device=qkv.device)
    ws = _ws(lib.th_attention_train_workspace_bytes(V, N, heads), qkv.device)
    _check(lib.th_attention_train(ctx(qkv.device), _p(qkv), V, N, heads, int(form), _p(out), _p(lse), _p(ws), ws.numel(),
                                  _stream()))
    return out, lse


def attention_bwd(qkv, out, lse, g_out, heads=3):
    """th_attention_bwd: the gradient of attention() with respect to qkv, in qkv's layout, from the forward's out and lse and
    the gradient g_out [V, N, heads * 64] of its output.  Nothing N x N is stored; bit-identical from run to run."""
    lib = load_library()
    qkv, out, lse, g_out = _f32(qkv), _f32(out), _f32(lse), _f32(g_out)
    V, N = _attn_dims(qkv, heads)
    if tuple(out.shape) != (V, N, heads * 64) or tuple(g_out.shape) != (V, N, heads * 64) or tuple(lse.shape) != (V, heads, N):
        raise ValueError(f"attention_bwd: out / g_out must be [{V}, {N}, {heads * 64}] and lse [{V}, {heads}, {N}]")
    g_qkv = torch.empty_like(qkv)
    ws = _ws(lib.th_attention_bwd_workspace_bytes(V, N, heads), qkv.device)
    _check(lib.th_attention_bwd(ctx(qkv.device), _p(qkv), _p(out), _p(lse), _p(g_out), V, N, heads, _p(g_qkv), _p(ws),
                                ws.numel(), _stream()))
    return g_qkv


OPERAND_PLAIN, OPERAND_LN, OPERAND_GELU = 0, 1, 2      # the operand forms of th_linear_train_forward / th_linear_bwd


def wgrad_chunk_rows():
    """rows per partial tile of the weight-gradient kernel (the chunks are added in order)"""
    return int(load_library().th_wgrad_chunk_rows())


def layernorm_bwd_chunk_rows():
    return int(load_library().th_layernorm_bwd_chunk_rows())


# ---------------------------------------------------------------------------
# K23: the backward of the encoder trunk (k_encoder_bwd.hip); NCHW fp32
# ---------------------------------------------------------------------------
def conv2d_bwd_supported(cin, cout, ks, stride):
    """th_conv2d_bwd_supported: 0, or bit 0: conv2d_wgrad is built for this convolution, bit 1: conv2d_dgrad as well"""
    return int(load_library().th_conv2d_bwd_supported(int(cin), int(cout), int(ks), int(stride)))


def conv2d_wgrad_chunk_pixels():
    return int(load_library().th_conv2d_wgrad_chunk_pixels())


def conv2d_dgrad_tile():
    """(rows, columns) of input pixels of one parity class that a workgroup of conv2d_dgrad owns"""
    lib = load_library()
    return int(lib.th_conv2d_dgrad_tile_rows()), int(lib.th_conv2d_dgrad_tile_cols())


def bn_act_bwd_slice_elems():
    return int(load_library().th_bn_act_bwd_slice_elems())


def _nchw(fn, name, t, channels=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype is torch.float32 and t.dim() == 4 and t.is_contiguous()):
        raise ValueError(f"{fn}: '{name}' must be a contiguous float32 [N,C,H,W] device tensor")
    if channels is not None and t.shape[1] != channels:
        raise ValueError(f"{fn}: '{name}' has {t.shape[1]} channels, expected {channels}")
    return t.detach()


def _conv_out(n, ks, stride):
    return (n + 2 * (ks // 2) - ks) // stride + 1


def _conv_weight(fn, weight):
    if not (weight.is_cuda and weight.dtype is torch.float32 and weight.dim() == 4 and weight.is_contiguous()
            and weight.shape[2] == weight.shape[3]):
        raise ValueError(f"{fn}: the weight must be a contiguous float32 [cout, cin, ks, ks] device tensor")
    return weight.detach(), int(weight.shape[1]), int(weight.shape[0]), int(weight.shape[2])


def conv2d_dgrad_pack(weight, stride):
    """th_conv2d_dgrad_pack: the image of `weight` [cout, cin, ks, ks] that conv2d_dgrad reads (one block per input-parity class)"""
    lib = load_library()
    w, cin, cout, ks = _conv_weight("conv2d_dgrad_pack", weight)
    n = int(lib.th_conv2d_dgrad_pack_bytes(cin, cout, ks, int(stride)))
    if n == 0:
        raise HipError(f"conv2d_dgrad_pack: no input gradient is built for a {ks}x{ks}/{stride} convolution {cin}->{cout}")
    packed = torch.empty(n, dtype=torch.uint8, device=w.device)
    _check(lib.th_conv2d_dgrad_pack(ctx(w.device), _p(w), cin, cout, ks, int(stride), _p(packed), n, _stream()))
    return packed


_dgrad_images = {}      # id(weight) -> (weakref, version, data_ptr, stride, packed)


def conv2d_dgrad_image(weight, stride):
    """the packed image of a Parameter, made once per weight version (an optimiser step bumps it)"""
    import weakref
    ent = _dgrad_images.get(id(weight))
    if ent is not None and ent[0]() is weight and ent[1:4] == (weight._version, weight.data_ptr(), int(stride)):
        return ent[4]
    if len(_dgrad_images) > 64:
        _dgrad_images.clear()
    packed = conv2d_dgrad_pack(weight, stride)
    _dgrad_images[id(weight)] = (weakref.ref(weight), weight._version, weight.data_ptr(), int(stride), packed)
    return packed


def conv2d_dgrad(g_y, weight_shape, stride, in_hw, packed):
    """th_conv2d_dgrad: g_y [N,cout,Ho,Wo] -> g_x [N,cin,H,W] for the convolution whose weight has `weight_shape` and whose input
    was H x W = `in_hw`; `packed` = conv2d_dgrad_pack(weight, stride).  Bit-identical from run to run."""
    lib = load_library()
    cout, cin, ks = int(weight_shape[0]), int(weight_shape[1]), int(weight_shape[2])
    H, W = int(in_hw[0]), int(in_hw[1])
    g = _nchw("conv2d_dgrad", "g_y", g_y, cout)
    if tuple(g.shape[2:]) != (_conv_out(H, ks, stride), _conv_out(W, ks, stride)):
        raise ValueError(f"conv2d_dgrad: g_y is {tuple(g.shape[2:])}, a {ks}x{ks}/{stride} convolution of {H}x{W} gives "
                         f"{(_conv_out(H, ks, stride), _conv_out(W, ks, stride))}")
    N = int(g.shape[0])
    g_x = torch.empty((N, cin, H, W), dtype=torch.float32, device=g.device)
    _check(lib.th_conv2d_dgrad(ctx(g.device), _p(g), N, cin, cout, ks, int(stride), H, W, _p(packed), packed.numel(), _p(g_x),
                               _stream()))
    return g_x


def conv2d_wgrad(x, g_y, ks, stride):
    """th_conv2d_wgrad: x [N,cin,H,W], g_y [N,cout,Ho,Wo] -> g_W [cout,cin,ks,ks].  Bit-identical from run to run."""
    lib = load_library()
    x2, g = _nchw("conv2d_wgrad", "x", x), _nchw("conv2d_wgrad", "g_y", g_y)
    N, cin, H, W = (int(n) for n in x2.shape)
    cout = int(g.shape[1])
    if tuple(g.shape) != (N, cout, _conv_out(H, ks, stride), _conv_out(W, ks, stride)):
        raise ValueError(f"conv2d_wgrad: g_y is {tuple(g.shape)}, expected "
                         f"{(N, cout, _conv_out(H, ks, stride), _conv_out(W, ks, stride))}")
    g_w = torch.empty((cout, cin, ks, ks), dtype=torch.float32, device=x2.device)
    ws = _ws(lib.th_conv2d_wgrad_workspace_bytes(N, cin, cout, int(ks), int(stride), H, W), x2.device)
    _check(lib.th_conv2d_wgrad(ctx(x2.device), _p(x2), _p(g), N, cin, cout, int(ks), int(stride), H, W, _p(g_w), _p(ws), ws.numel(),
                               _stream()))
    return g_w


def bn_act_bwd(y, out, g, gamma, eps, need_residual=False, need_affine=True):
    """th_bn_act_bwd: the backward of train-mode BatchNorm (+ residual) (+ ReLU).  y: the BatchNorm's input, out: the site's
    output (None: the site has no ReLU), g: the gradient of the site's output, gamma: [C] or None (1) ->
    (g_y, g_residual or None, g_gamma or None, g_beta or None).  Bit-identical from run to run."""
    lib = load_library()
    fn = "bn_act_bwd"
    y2, g2 = _nchw(fn, "y", y), _nchw(fn, "g", g)
    o2 = None if out is None else _nchw(fn, "out", out)
    if g2.shape != y2.shape or (o2 is not None and o2.shape != y2.shape):
        raise ValueError(f"{fn}: y, out and g must have one shape")
    N, Cc, H, W = (int(n) for n in y2.shape)
    gm = None if gamma is None else _train_vec(fn, gamma, Cc)
    g_y = torch.empty_like(y2)
    g_res = torch.empty_like(y2) if need_residual else None
    g_gamma = torch.empty(Cc, dtype=torch.float32, device=y2.device) if need_affine else None
    g_beta = torch.empty(Cc, dtype=torch.float32, device=y2.device) if need_affine else None
    ws = _ws(lib.th_bn_act_bwd_workspace_bytes(N, Cc, H * W), y2.device)
    _check(lib.th_bn_act_bwd(ctx(y2.device), _p(y2), _p(o2), _p(g2), N, Cc, H * W, _p(gm), float(eps), _p(g_y), _p(g_res),
                             _p(g_gamma), _p(g_beta), _p(ws), ws.numel(), _stream()))
    return g_y, g_res, g_gamma, g_beta


BN_RECORD = 6       # a0 a1 a2 a3 p L per channel (th_bn_act_bwd_sums)


def _bn_site(fn, y, out, g):
    y2, g2 = _nchw(fn, "y", y), _nchw(fn, "g", g)
    o2 = None if out is None else _nchw(fn, "out", out)
    if g2.shape != y2.shape or (o2 is not None and o2.shape != y2.shape):
        raise ValueError(f"{fn}: y, out and g must have one shape")
    return y2, o2, g2


def bn_act_bwd_sums(y, out, g):
    """th_bn_act_bwd_sums: pass A of bn_act_bwd over this rank's batch -> the rank's record, float64 [C, 6] = a0 a1 a2 a3 p L
    on the device, for the all_gather of a SyncBatchNorm site"""
    lib = load_library()
    y2, o2, g2 = _bn_site("bn_act_bwd_sums", y, out, g)
    N, Cc, H, W = (int(n) for n in y2.shape)
    record = torch.empty((Cc, BN_RECORD), dtype=torch.float64, device=y2.device)
    ws = _ws(lib.th_bn_act_bwd_workspace_bytes(N, Cc, H * W), y2.device)
    _check(lib.th_bn_act_bwd_sums(ctx(y2.device), _p(y2), _p(o2), _p(g2), N, Cc, H * W, _p(record), _p(ws), ws.numel(), _stream()))
    return record


def bn_act_bwd_apply(y, out, g, gamma, eps, records, rank, need_residual=False, need_affine=True):
    """th_bn_act_bwd_apply: ``records`` float64 [world, C, 6], the ranks' bn_act_bwd_sums in rank order; y, out, g are rank
    ``rank``'s -> (g_y, g_residual or None, g_gamma or None, g_beta or None) as bn_act_bwd, with the statistics of all ranks and
    the LOCAL g_gamma / g_beta.  world 1 is bn_act_bwd bit for bit."""
    lib = load_library()
    fn = "bn_act_bwd_apply"
    y2, o2, g2 = _bn_site(fn, y, out, g)
    N, Cc, H, W = (int(n) for n in y2.shape)
    if not (isinstance(records, torch.Tensor) and records.dtype is torch.float64 and records.dim() == 3 and records.is_contiguous()
            and records.device == y2.device and tuple(records.shape[1:]) == (Cc, BN_RECORD)):
        raise ValueError(f"{fn}: 'records' must be a contiguous float64 [world, {Cc}, {BN_RECORD}] tensor on {y2.device}")
    world = int(records.shape[0])
    gm = None if gamma is None else _train_vec(fn, gamma, Cc)
    g_y = torch.empty_like(y2)
    g_res = torch.empty_like(y2) if need_residual else None
    g_gamma = torch.empty(Cc, dtype=torch.float32, device=y2.device) if need_affine else None
    g_beta = torch.empty(Cc, dtype=torch.float32, device=y2.device) if need_affine else None
    _check(lib.th_bn_act_bwd_apply(ctx(y2.device), _p(y2), _p(o2), _p(g2), N, Cc, H * W, _p(gm), float(eps), _p(records), world,
                                   int(rank), _p(g_y), _p(g_res), _p(g_gamma), _p(g_beta), _stream()))
    return g_y, g_res, g_gamma, g_beta


def maxpool3x3s2_bwd(x, g):
    """th_maxpool3x3s2_bwd: x [N,C,H,W] (the input of nn.MaxPool2d(3, 2, 1)), g [N,C,Ho,Wo] -> g_x; torch's routing rule"""
    x2, g2 = _nchw("maxpool3x3s2_bwd", "x", x), _nchw("maxpool3x3s2_bwd", "g", g)
    N, Cc, H, W = (int(n) for n in x2.shape)
    if tuple(g2.shape) != (N, Cc, (H - 1) // 2 + 1, (W - 1) // 2 + 1):
        raise ValueError(f"maxpool3x3s2_bwd: g is {tuple(g2.shape)}, expected {(N, Cc, (H - 1) // 2 + 1, (W - 1) // 2 + 1)}")
    g_x = torch.empty_like(x2)
    _check(load_library().th_maxpool3x3s2_bwd(ctx(x2.device), _p(x2), _p(g2), N * Cc, H, W, _p(g_x), _stream()))
    return g_x


# ---------------------------------------------------------------------------
# K29: the forward convolutions of the encoder trunk in training (k_encoder_fwd.hip); NCHW fp32
# ---------------------------------------------------------------------------
def conv2d_fwd32_supported(cin, cout, ks, stride):
    """th_conv2d_fwd32_supported: True for the five convolutions of the trunk conv2d_fwd32 is built for"""
    return bool(load_library().th_conv2d_fwd32_supported(int(cin), int(cout), int(ks), int(stride)))


def conv2d_fwd32_tile():
    """(rows, columns) of output pixels that a workgroup of conv2d_fwd32 owns"""
    lib = load_library()
    return int(lib.th_conv2d_fwd32_tile_rows()), int(lib.th_conv2d_fwd32_tile_cols())


def conv2d_fwd32_chunk_channels():
    return int(load_library().th_conv2d_fwd32_chunk_channels())


def conv2d_fwd32(x, weight, stride):
    """th_conv2d_fwd32: nn.Conv2d(cin, cout, ks, stride, ks // 2, bias=False) on x [N,cin,H,W] with torch's weight
    [cout,cin,ks,ks] -> y [N,cout,Ho,Wo], exact fp32 operands on the MFMA, fixed-order sums.  Bit-identical from run to run."""
    lib = load_library()
    x2 = _nchw("conv2d_fwd32", "x", x)
    w, cin, cout, ks = _conv_weight("conv2d_fwd32", weight)
    if x2.shape[1] != cin or w.device != x2.device:
        raise ValueError(f"conv2d_fwd32: 'x' has {x2.shape[1]} channels on {x2.device}, the weight takes {cin} on {w.device}")
    N, _, H, W = (int(n) for n in x2.shape)
    st = int(stride)
    if not lib.th_conv2d_fwd32_supported(cin, cout, ks, st):
        raise HipError(f"conv2d_fwd32: no HIP forward is built for a {ks}x{ks}/{st} convolution {cin}->{cout}")
    y = torch.empty((N, cout, _conv_out(H, ks, st), _conv_out(W, ks, st)), dtype=torch.float32, device=x2.device)
    _check(lib.th_conv2d_fwd32(ctx(x2.device), _p(x2), N, cin, H, W, _p(w), cout, ks, st, _p(y), _stream()))
    return y


# ---------------------------------------------------------------------------
# K22: the optimiser step (th_adam_plan / th_adam_step)
# ---------------------------------------------------------------------------
ADAM_CLIP, ADAM_ZERO_GRAD, ADAM_COUNT_NONFINITE, ADAM_CHECK_POINTERS, ADAM_T_DECOUPLED = (
    _H.constants["TH_" + n] for n in ("ADAM_CLIP", "ADAM_ZERO_GRAD", "ADAM_COUNT_NONFINITE", "ADAM_CHECK_POINTERS",
                                      "ADAM_T_DECOUPLED"))
# th_adam_tensor as a numpy record: the per-step table is filled column-wise, not entry by entry
ADAM_TENSOR_FIELDS = _H.records["th_adam_tensor"]


def adam_chunk_elems():
    """elements per workgroup of adam_step_kernel (a tensor's last chunk holds the rest)"""
    return int(load_library().th_adam_chunk_elems())


def adam_flat_layout(counts, live=None):
    """th_adam_flat_layout (a pure host call) -> (offsets, flat_elems): where each tensor's slot starts in the flat buffer of the
    gradient exchange (-1: no slot) and the buffer's length; ``live``: one truth value per tensor, None for all"""
    import numpy as np
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    offsets = np.empty(len(counts), dtype=np.int64)
    lv = None if live is None else np.ascontiguousarray(np.asarray(live) != 0, dtype=np.uint8)
    if lv is not None and lv.shape != counts.shape:
        raise HipError("adam_flat_layout: one entry of `live` per tensor")
    end = int(load_library().th_adam_flat_layout(len(counts), counts.ctypes.data, None if lv is None else lv.ctypes.data,
                                                 offsets.ctypes.data))
    if end < 0:
        raise HipError("adam_flat_layout: sizes out of range")
    return offsets, end


def rank_sum(parts, world, slice_elems, out):
    """th_rank_sum (K28): out[e] = ((parts[0][e] + parts[1][e]) + ...) in fp32, in rank order.  ``parts``: a contiguous fp32 device
    tensor of at least world * slice_elems elements, read as [world, slice_elems]; ``out``: at least slice_elems elements, and may
    be the view of any one part."""
    world, slice_elems = int(world), int(slice_elems)
    for name, t, need in (("parts", parts, max(world, 1) * slice_elems), ("out", out, slice_elems)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype is torch.float32 and t.is_contiguous()):
            raise HipError(f"rank_sum: '{name}' must be a contiguous float32 device tensor (there is no CPU path)")
        if t.numel() < need:
            raise HipError(f"rank_sum: '{name}' holds {t.numel()} elements, the call reads or writes {need}")
    if out.device != parts.device:
        raise HipError("rank_sum: parts and out live on different devices")
    with torch.cuda.device(parts.device):
        _check(load_library().th_rank_sum(ctx(parts.device), _p(parts), world, slice_elems, _p(out), _stream()))
    return out


def adam_check_tensor(t, what):
    """the refusals of the optimiser step that a raw pointer cannot show: HipError, nothing is converted silently"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise HipError(f"adam_step: {what} is not a device tensor (there is no CPU path)")
    if t.dtype is not torch.float32:
        raise HipError(f"adam_step: {what} is {t.dtype}, the kernel updates fp32 only")
    if not t.is_contiguous():
        raise HipError(f"adam_step: {what} is not contiguous")


class AdamPlan:
    """th_adam_plan for a fixed list of contiguous fp32 device tensors: owns the device tables and the pinned ring."""

    def __init__(self, params):
        import numpy as np
        lib = load_library()
        params = list(params)
        if not params:
            raise HipError("adam_plan: no tensors")
        for i, p in enumerate(params):
            adam_check_tensor(p, f"parameter {i}")
            if p.numel() == 0:
                raise HipError(f"adam_plan: parameter {i} has no elements")
            if p.device != params[0].device:
                raise HipError("adam_plan: the parameters live on different devices")
        self.device = params[0].device
        self.n = len(params)
        counts = np.array([p.numel() for p in params], dtype=np.int64)
        self.counts = [int(n) for n in counts]
        ptrs = np.array([p.data_ptr() for p in params], dtype=np.uint64)
        nbytes = int(lib.th_adam_table_bytes(self.n, int(counts.sum())))
        if nbytes == 0:
            raise HipError("adam_plan: sizes out of range")
        self.table = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.dtype = np.dtype(ADAM_TENSOR_FIELDS)
        assert self.dtype.itemsize == lib.th_sizeof(b"th_adam_tensor")
        self.steps = 0
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _check(lib.th_adam_plan(ctx(self.device), self.n, counts.ctypes.data, ptrs.ctypes.data, _p(self.table),
                                    nbytes, C.byref(h), _stream()))
        self._h = h
        self._destroy = lib.th_adam_plan_destroy

    def step(self, table, clip=None, zero_grad=False, count_nonfinite=False, check_pointers=False):
        """table: numpy records of ADAM_TENSOR_FIELDS, one per planned tensor (p = 0 skips a tensor)"""
        assert table.dtype == self.dtype and table.shape == (self.n,) and table.flags.c_contiguous
        flags = ((ADAM_CLIP if clip is not None else 0) | (ADAM_ZERO_GRAD if zero_grad else 0) |
                 (ADAM_COUNT_NONFINITE if count_nonfinite else 0) | (ADAM_CHECK_POINTERS if check_pointers else 0))
        clip = float(clip if clip is not None else 0.0)
        if torch._C._cuda_getDevice() == self.device.index:              # (the usual case: no context manager on the hot path)
            _check(_lib.th_adam_step(ctx(self.device), self._h, table.ctypes.data, self.n, clip, flags, None, _stream()))
        else:
            with torch.cuda.device(self.device):
                _check(_lib.th_adam_step(ctx(self.device), self._h, table.ctypes.data, self.n, clip, flags, None, _stream()))
        self.steps += 1

    def _flat_args(self, tensors, offsets, flat, flat_elems, what):
        import numpy as np
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if len(tensors) != self.n or offsets.shape != (self.n,):
            raise HipError(f"{what}: the plan holds {self.n} tensors")
        adam_check_tensor(flat, "the flat buffer")
        if flat.device != self.device or flat.numel() < flat_elems:
            raise HipError(f"{what}: the flat buffer holds {flat.numel()} elements on {flat.device}, not {flat_elems} on {self.device}")
        if isinstance(tensors, np.ndarray):                              # addresses the caller has checked before
            assert tensors.dtype == np.uint64 and tensors.flags.c_contiguous
            return tensors, offsets
        ptrs = np.zeros(self.n, dtype=np.uint64)
        for i, t in enumerate(tensors):
            if t is None or offsets[i] < 0:
                continue
            adam_check_tensor(t, f"tensor {i}")
            if t.numel() != self.counts[i] or t.device != self.device:
                raise HipError(f"{what}: tensor {i} has {t.numel()} elements on {t.device}, the plan {self.counts[i]} on {self.device}")
            ptrs[i] = t.data_ptr()
        return ptrs, offsets

    def _flat_call(self, fn, *args):
        if torch._C._cuda_getDevice() == self.device.index:
            _check(fn(ctx(self.device), self._h, *args, _stream()))
        else:
            with torch.cuda.device(self.device):
                _check(fn(ctx(self.device), self._h, *args, _stream()))

    def pack(self, grads, offsets, world, flat, flat_elems):
        """th_adam_pack: flat[offsets[i] + e] = grads[i][e] / world; grads[i] None writes zeros; offsets[i] < 0: no slot.  A
        gradient may be the view flat[offsets[i] : offsets[i] + n] itself.  ``grads`` may also be the uint64 array of addresses
        that an earlier call with the same tensors returned."""
        ptrs, offsets = self._flat_args(grads, offsets, flat, flat_elems, "adam_pack")
        self._flat_call(_lib.th_adam_pack, ptrs.ctypes.data, offsets.ctypes.data, self.n, int(world), _p(flat), int(flat_elems))
        return ptrs

    def unpack(self, dst, offsets, flat, flat_elems):
        """th_adam_unpack: dst[i][e] = flat[offsets[i] + e] for every tensor with a slot"""
        ptrs, offsets = self._flat_args(dst, offsets, flat, flat_elems, "adam_unpack")
        self._flat_call(_lib.th_adam_unpack, ptrs.ctypes.data, offsets.ctypes.data, self.n, _p(flat), int(flat_elems))

    def nonfinite(self):
        """gradient elements that were NaN or +-inf in the counted steps so far (synchronises the current stream)"""
        out = C.c_uint64(0)
        with torch.cuda.device(self.device):
            _check(_lib.th_adam_step(ctx(self.device), self._h, None, 0, 0.0, 0, C.byref(out), _stream()))
        return int(out.value)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and not sys.is_finalizing():          # (at interpreter exit the runtime may be gone already)
            try:
                self._destroy(h)
            except Exception:
                pass


def _train_rows(fn, t, cols=None):
    """a contiguous fp32 device tensor [..., cols] as rows [M, cols] (the training entries convert nothing silently)"""
    if not t.is_cuda:
        raise HipError(f"{fn} needs its tensors on an MI355X (there is no CPU path)")
    if t.dtype is not torch.float32 or not t.is_contiguous() or t.dim() < 1:
        raise ValueError(f"{fn}: tensors must be contiguous float32")
    if cols is not None and t.shape[-1] != cols:
        raise ValueError(f"{fn}: expected rows of {cols} values, got {t.shape[-1]}")
    return t.detach().reshape(-1, t.shape[-1])


def _train_vec(fn, t, n):
    if t is None:
        return None
    if not t.is_cuda:
        raise HipError(f"{fn} needs its tensors on an MI355X (there is no CPU path)")
    if t.dtype is not torch.float32 or not t.is_contiguous() or tuple(t.shape) != (n,):
        raise ValueError(f"{fn}: expected a contiguous float32 vector of {n} values")
    return t.detach()


def _dense_forward(fn, a, weight, bias, form=OPERAND_PLAIN, ln_w=None, ln_b=None, eps=1e-6, relu=False):
    """the one forward of a dense training layer: th_linear_train_forward, or with ``relu`` (form 0 only) th_linear_relu_forward"""
    lib = load_library()
    w = _train_rows(fn, weight)
    out_f, in_f = w.shape
    a2 = _train_rows(fn, a, in_f)
    b = _train_vec(fn, bias, out_f)
    lw, lb = _train_vec(fn, ln_w, in_f), _train_vec(fn, ln_b, in_f)
    M = a2.shape[0]
    lin = ThLinear(_p(w), _p(b), out_f, in_f)
    out = torch.empty((*a.shape[:-1], out_f), dtype=torch.float32, device=a.device)
    head = (ctx(a.device), _p(a2), in_f, M)
    tail = (C.byref(lin), _p(out), out_f)
    if relu:
        ws = _ws(lib.th_linear_relu_workspace_bytes(M, out_f, in_f), a.device)
        _check(lib.th_linear_relu_forward(*head, *tail, _p(ws), ws.numel(), _stream()))
    else:
        ws = _ws(lib.th_linear_train_workspace_bytes(M, out_f, in_f, int(form)), a.device)
        _check(lib.th_linear_train_forward(*head, int(form), _p(lw), _p(lb), float(eps), *tail, _p(ws), ws.numel(), _stream()))
    return out


def _dense_bwd(fn, a, weight, g_out, form=OPERAND_PLAIN, ln_w=None, ln_b=None, eps=1e-6, y=None, need_input=True,
               need_bias=True):
    """the one backward of a dense training layer: th_linear_bwd, or with the output ``y`` of a ReLU layer (form 0 only)
    th_linear_relu_bwd -> (g_a or None, g_W, g_b or None, g_ln_w, g_ln_b)"""
    lib = load_library()
    w = _train_rows(fn, weight)
    out_f, in_f = w.shape
    a2, g2 = _train_rows(fn, a, in_f), _train_rows(fn, g_out, out_f)
    y2 = None if y is None else _train_rows(fn, y, out_f)
    M = a2.shape[0]
    if g2.shape[0] != M or (y2 is not None and y2.shape[0] != M):
        rows = "" if y2 is None else f"{y2.shape[0]} output rows, "
        raise ValueError(f"{fn}: {M} operand rows, {rows}{g2.shape[0]} gradient rows")
    lw, lb = _train_vec(fn, ln_w, in_f), _train_vec(fn, ln_b, in_f)
    lin = ThLinear(_p(w), None, out_f, in_f)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=a.device)
    g_a = new(*a.shape) if need_input else None
    g_w = new(out_f, in_f)
    g_b = new(out_f) if need_bias else None
    ln = need_input and int(form) == OPERAND_LN
    g_lw, g_lb = (new(in_f), new(in_f)) if ln else (None, None)
    grads = (_p(g2), out_f, _p(g_a), in_f, _p(g_w), _p(g_b))
    if y is None:
        ws = _ws(lib.th_linear_bwd_workspace_bytes(M, out_f, in_f, int(form)), a.device)
        _check(lib.th_linear_bwd(ctx(a.device), _p(a2), in_f, M, int(form), _p(lw), _p(lb), float(eps), C.byref(lin), *grads,
                                 _p(g_lw), _p(g_lb), _p(ws), ws.numel(), _stream()))
    else:
        ws = _ws(lib.th_linear_relu_bwd_workspace_bytes(M, out_f, in_f), a.device)
        _check(lib.th_linear_relu_bwd(ctx(a.device), _p(a2), in_f, _p(y2), out_f, M, C.byref(lin), *grads, _p(ws), ws.numel(),
                                      _stream()))
    return g_a, g_w, g_b, g_lw, g_lb


def linear_train_forward(a, weight, bias, form=OPERAND_PLAIN, ln_w=None, ln_b=None, eps=1e-6):
    """th_linear_train_forward: op(a) W^T + b with op = identity / LayerNorm / gelu (form), a [..., in] -> [..., out]"""
    return _dense_forward("linear_train_forward", a, weight, bias, form, ln_w, ln_b, eps)


def linear_bwd(a, weight, g_out, form=OPERAND_PLAIN, ln_w=None, ln_b=None, eps=1e-6, need_input=True, need_bias=True):
    """th_linear_bwd: the gradients of linear_train_forward from g_out [..., out] -> (g_a or None, g_W, g_b or None, g_ln_w,
    g_ln_b); the last two are None unless form = OPERAND_LN with need_input.  g_a is the gradient of `a` itself (through the
    LayerNorm / the gelu).  Bit-identical from run to run."""
    return _dense_bwd("linear_bwd", a, weight, g_out, form, ln_w, ln_b, eps, need_input=need_input, need_bias=need_bias)


def linear_relu_forward(a, weight, bias):
    """th_linear_relu_forward: relu(a W^T + b), a [..., in] -> [..., out] (the ReLU in the GEMM's epilogue)"""
    return _dense_forward("linear_relu_forward", a, weight, bias, relu=True)


def linear_relu_bwd(a, y, weight, g_out, need_input=True, need_bias=True):
    """th_linear_relu_bwd: the gradients of linear_relu_forward from its output y and g_out [..., out] -> (g_a or None, g_W,
    g_b or None).  Bit-identical from run to run."""
    return _dense_bwd("linear_relu_bwd", a, weight, g_out, y=y, need_input=need_input, need_bias=need_bias)[:3]


def _xview_rows(fn, kvp, kvs):
    a, b = _train_rows(fn, kvp, 384), _train_rows(fn, kvs, 384)
    if kvp.dim() != 3 or kvp.shape != kvs.shape or not 1 <= kvp.shape[1] <= 4 or kvp.shape[0] < 1:
        raise ValueError(f"{fn}: kvp and kvs must both be [P, V, 384] with P >= 1 and V in 1..4")
    return a, b, int(kvp.shape[0]), int(kvp.shape[1])


def xview_attention(kvp, kvs):
    """th_xview_attention: the rows [key(128) | value(256)] of the pixel and token branch, [P,V,384] each -> n [P,V,256]"""
    lib = load_library()
    a, b, P, V = _xview_rows("xview_attention", kvp, kvs)
    n = torch.empty((P, V, 256), dtype=torch.float32, device=kvp.device)
    _check(lib.th_xview_attention(ctx(kvp.device), _p(a), _p(b), P, V, _p(n), _stream()))
    return n


def xview_attention_bwd(kvp, kvs, g_n):
    """th_xview_attention_bwd: g_n [P,V,256] -> (g_kvp, g_kvs) [P,V,384]; bit-identical from run to run"""
    lib = load_library()
    fn = "xview_attention_bwd"
    a, b, P, V = _xview_rows(fn, kvp, kvs)
    g = _train_rows(fn, g_n, 256)
    if tuple(g_n.shape) != (P, V, 256):
        raise ValueError(f"{fn}: g_n must be [{P}, {V}, 256]")
    g_kvp, g_kvs = torch.empty_like(kvp), torch.empty_like(kvs)
    _check(lib.th_xview_attention_bwd(ctx(kvp.device), _p(a), _p(b), _p(g), P, V, _p(g_kvp), _p(g_kvs), _stream()))
    return g_kvp, g_kvs


def layernorm_train_forward(x, weight, bias, eps=1e-6):
    """th_layernorm_forward: LayerNorm over the last dimension with the statistics rule of the LayerNorm-fused GEMM"""
    lib = load_library()
    fn = "layernorm_train_forward"
    dim = x.shape[-1]
    x2, w, b = _train_rows(fn, x), _train_vec(fn, weight, dim), _train_vec(fn, bias, dim)
    out = torch.empty_like(x2)
    _check(lib.th_layernorm_forward(ctx(x.device), _p(x2), dim, x2.shape[0], dim, _p(w), _p(b), float(eps), _p(out), dim,
                                    _stream()))
    return out.reshape(x.shape)


def layernorm_bwd(x, weight, g_out, eps=1e-6):
    """th_layernorm_bwd -> (g_x, g_w, g_b); bit-identical from run to run"""
    lib = load_library()
    fn = "layernorm_bwd"
    dim = x.shape[-1]
    x2, g2, w = _train_rows(fn, x), _train_rows(fn, g_out, dim), _train_vec(fn, weight, dim)
    if x2.shape != g2.shape:
        raise ValueError(f"{fn}: x and g_out differ in shape")
    M = x2.shape[0]
    g_x = torch.empty_like(x2)
    g_w, g_b = (torch.empty((dim,), dtype=torch.float32, device=x.device) for _ in range(2))
    ws = _ws(lib.th_layernorm_bwd_workspace_bytes(M, dim), x.device)
    _check(lib.th_layernorm_bwd(ctx(x.device), _p(x2), dim, M, dim, _p(w), float(eps), _p(g2), dim, _p(g_x), dim, _p(g_w),
                                _p(g_b), _p(ws), ws.numel(), _stream()))
    return g_x.reshape(x.shape), g_w, g_b


def dparf_encode(pts_smpl, centres, rot, tokens, sel=None):
    lib = load_library()
    p, c, r, t = _f32(pts_smpl).reshape(-1, 3), _f32(centres).reshape(-1, 3), _f32(rot).reshape(-1, 9), _f32(tokens)
    P = p.shape[0] if sel is None else sel.numel()
    V, nc = t.shape[0], t.shape[1]
    out = torch.empty((P, V, 256), dtype=torch.float32, device=p.device)
    _check(lib.th_dparf_encode(ctx(p.device), _p(p), _p(sel), P, _p(c), _p(r), _p(t), V, nc, _p(out), _stream()))
    return out


def nchw_to_nhwc(m):
    lib = load_library()
    m = _f32(m)
    V, Cc, H, W = m.shape
    out = torch.empty((V, H, W, Cc), dtype=torch.float32, device=m.device)
    _check(lib.th_nchw_to_nhwc(ctx(m.device), _p(m), V, Cc, H, W, _p(out), _stream()))
    return out


def pixel_gather(map_nhwc, pts_world, cams, scale_xy, sel=None, row_floats=None):
    """-> [P, V, row_floats] (default: the map's channel count; wider rows are zero padded)."""
    lib = load_library()
    V, H, W, Cc = map_nhwc.shape
    p = _f32(pts_world).reshape(-1, 3)
    P = p.shape[0] if sel is None else sel.numel()
    ldo = Cc if row_floats is None else int(row_floats)
    out = torch.empty((P, V, ldo), dtype=torch.float32, device=p.device)
    _check(lib.th_pixel_gather(ctx(p.device), _p(map_nhwc), V, Cc, H, W, _p(p), _p(sel), P, _p(cams), _p(scale_xy),
                               _p(out), ldo, _stream()))
    return out


def pixel_gather_split(split_map, pts_world, cams, scale_xy, sel=None):
    """th_pixel_gather_split: the split-row form of the pixel-aligned gather (what the frame-level entry points run) ->
    (hi, lo) fp16 tensors [P, V, 272] (x = hi + lo), decoded from the [8 hi | 8 lo] groups of the rows."""
    lib = load_library()
    assert isinstance(split_map, SplitMap)
    V, H, W = split_map.V, split_map.H, split_map.W
    p = _f32(pts_world).reshape(-1, 3)
    P = p.shape[0] if sel is None else sel.numel()
    out = torch.zeros((P, V, 272 * 2), dtype=torch.float16, device=p.device)
    _check(lib.th_pixel_gather_split(ctx(p.device), _p(split_map), V, H, W, _p(p), _p(sel), P, _p(cams), _p(scale_xy),
                                     _p(out), 272, _stream()))
    g = out.view(P, V, 34, 2, 8)
    return g[:, :, :, 0].reshape(P, V, 272), g[:, :, :, 1].reshape(P, V, 272)


def pixel_texlist(split_map, pts_world, cams, scale_xy, sel=None):
    """th_pixel_texlist: K5t on its own -> dict(lists [T,4,128] int32, records [T,V,32,8] int32 (float bits / byte offsets)),
    T = ceil(P / 32) tiles of 32 consecutive samples."""
    lib = load_library()
    assert isinstance(split_map, SplitMap)
    V, H, W = split_map.V, split_map.H, split_map.W
    p = _f32(pts_world).reshape(-1, 3)
    P = p.shape[0] if sel is None else sel.numel()
    T = (P + 31) // 32
    nb = int(lib.th_pixel_texlist_bytes(V, P))
    out = torch.zeros(nb // 4, dtype=torch.int32, device=p.device)
    _check(lib.th_pixel_texlist(ctx(p.device), _p(split_map), V, H, W, _p(p), _p(sel), P, _p(cams), _p(scale_xy), _p(out), nb,
                                _stream()))
    a, b = T * 512, T * 512 + T * V * 32 * 8
    return dict(lists=out[:a].view(T, 4, 128), records=out[a:b].view(T, V, 32, 8))


def network_forward(net, pixel_feat, viewdir, pts_smpl, centres, rot, tokens, mask=None):
    """Network.forward on gathered inputs -> raw [P,4]."""
    lib = load_library()
    _sync_weights(net, "mlp")
    pf, vd, ps = _f32(pixel_feat), _f32(viewdir).reshape(-1, 27), _f32(pts_smpl).reshape(-1, 3)
    V, Cc, P = pf.shape
    assert Cc == 384 and vd.shape[0] == P and ps.shape[0] == P
    c, r, t = _f32(centres).reshape(-1, 3), _f32(rot).reshape(-1, 9), _f32(tokens)
    m = mask.reshape(-1).to(torch.uint8).contiguous() if mask is not None else None
    raw = torch.empty((P, 4), dtype=torch.float32, device=pf.device)
    if P == 0:
        return raw
    ws = _ws(lib.th_network_workspace_bytes(V, P), pf.device)
    def launch(_frame, _i):
        _check(lib.th_network_forward(ctx(pf.device), _p(pf), _p(vd), _p(ps), _p(m), P, _p(c), _p(r), _p(t), V, t.shape[1],
                                      _p(raw), _p(ws), ws.numel(), _stream()))
        return lib.th_range_last_slot(ctx(pf.device))
    _guarded(pf.device, launch, 3)                   # (a switch: the context is on the fp32 path now -- run again)
    return raw


def composite(raw, z, ray_d, white_bkgd=False, return_weights=False):
    lib = load_library()
    raw, z, d = _f32(raw), _f32(z), _f32(ray_d).reshape(-1, 3)
    R, S = z.shape
    pts = ThPoints(None, None, _p(d), None, None, None, None, R, S)
    rgb = torch.empty((R, 3), dtype=torch.float32, device=raw.device)
    acc = torch.empty(R, dtype=torch.float32, device=raw.device)
    dep = torch.empty(R, dtype=torch.float32, device=raw.device)
    w = torch.empty((R, S), dtype=torch.float32, device=raw.device) if return_weights else None
    _check(lib.th_composite(ctx(raw.device), _p(raw), _p(z), C.byref(pts), int(white_bkgd), _p(rgb), _p(acc), _p(dep),
                            _p(w), _stream()))
    return (rgb, acc, dep, w) if return_weights else (rgb, acc, dep)


def dparf_encode_bwd(pts_smpl, centres, rot, grad_out, out=None):
    """th_dparf_encode_bwd: grad_out [P,V,256] -> grad_tokens [V,N_c,192], the adjoint of dparf_encode with respect to the
    tokens.  ``out`` (optional) is written in full."""
    lib = load_library()
    p, c, r, g = _f32(pts_smpl).reshape(-1, 3), _f32(centres).reshape(-1, 3), _f32(rot).reshape(-1, 9), _f32(grad_out)
    P, V = g.shape[0], g.shape[1]
    assert g.shape == (P, V, 256) and p.shape[0] == P
    nc = c.shape[0]
    if out is None:
        out = torch.empty((V, nc, 192), dtype=torch.float32, device=c.device)
    assert out.shape == (V, nc, 192) and out.dtype is torch.float32 and out.is_contiguous()
    ws = _ws(lib.th_dparf_encode_bwd_workspace_bytes(P, V, nc), c.device)
    _check(lib.th_dparf_encode_bwd(ctx(c.device), _p(p), P, _p(c), _p(r), V, nc, _p(g), _p(out), _p(ws), ws.numel(), _stream()))
    return out


def pixel_gather_bwd(map_shape, pts_world, cams, scale_xy, grad_out, out=None):
    """th_pixel_gather_bwd: grad_out [P,V,ldo] -> grad_map [V,H,W,C] (map_shape), the adjoint of pixel_gather with respect
    to the map.  ``out`` (optional) is written in full."""
    lib = load_library()
    V, H, W, Cc = (int(x) for x in map_shape)
    p, g = _f32(pts_world).reshape(-1, 3), _f32(grad_out)
    P, ldo = p.shape[0], g.shape[-1]
    assert g.shape == (P, V, ldo)
    if out is None:
        out = torch.empty((V, H, W, Cc), dtype=torch.float32, device=g.device)
    assert out.shape == (V, H, W, Cc) and out.dtype is torch.float32 and out.is_contiguous()
    _check(lib.th_pixel_gather_bwd(ctx(g.device), V, Cc, H, W, _p(p), P, _p(cams), _p(scale_xy), _p(g), ldo, _p(out), _stream()))
    return out


def _latent_dims(shapes):
    """[(V,h,w,C)] x 3 -> the int32[6] {h0,w0,h1,w1,h2,w2} of th_latent_gather"""
    (V, h0, w0, c0), (V1, h1, w1, c1), (V2, h2, w2, c2) = (tuple(int(x) for x in sh) for sh in shapes)
    if (c0, c1, c2) != (64, 64, 128) or V1 != V or V2 != V:
        raise ValueError(f"latent_gather: channels-last latents [V,h,w,64], [V,h,w,64], [V,h,w,128] expected, not {list(shapes)}")
    return V, (C.c_int32 * 6)(h0, w0, h1, w1, h2, w2)


def _channels_last_latent(t):
    if t.dtype is not torch.float32 or not t.is_contiguous() or t.dim() != 4:
        raise ValueError("latent_gather: every latent must be a contiguous float32 [V,h,w,C] tensor")
    return _f32(t)


def latent_gather(lat0, lat1, lat2, lift_w, lift_b, images, pts_world, cams, scale_xy, row_floats=384):
    """th_latent_gather: the 384-channel pixel feature at the projected points, read from the channels-last latents
    [V,h,w,64 | 64 | 128] and the images [V,3,H,W] -> (rows [P,V,row_floats], rgb_s [P,V,4])."""
    lib = load_library()
    l0, l1, l2 = (_channels_last_latent(t) for t in (lat0, lat1, lat2))
    V, dims = _latent_dims((l0.shape, l1.shape, l2.shape))
    img = _f32(images)
    assert img.shape[0] == V and img.shape[1] == 3
    H, W = int(img.shape[2]), int(img.shape[3])
    p = _f32(pts_world).reshape(-1, 3)
    P, ldo = p.shape[0], int(row_floats)
    out = torch.empty((P, V, ldo), dtype=torch.float32, device=p.device)
    rgb_s = torch.empty((P, V, 4), dtype=torch.float32, device=p.device)
    _check(lib.th_latent_gather(ctx(p.device), _p(l0), _p(l1), _p(l2), dims, _p(img), _p(_f32(lift_w).reshape(128, 3)),
                                _p(_f32(lift_b).reshape(128)), V, H, W, _p(p), P, _p(cams), _p(scale_xy), _p(out), ldo,
                                _p(rgb_s), _stream()))
    return out, rgb_s


def latent_gather_bwd(latent_shapes, image_hw, pts_world, cams, scale_xy, grad_out, out=None):
    """th_latent_gather_bwd: grad_out [P,V,ldo] -> the gradients of the three channels-last latents (latent_shapes), the adjoint
    of latent_gather with respect to them.  ``out`` (optional, three tensors) is written in full."""
    lib = load_library()
    V, dims = _latent_dims(latent_shapes)
    H, W = (int(x) for x in image_hw)
    p, g = _f32(pts_world).reshape(-1, 3), _f32(grad_out)
    P, ldo = p.shape[0], g.shape[-1]
    assert g.shape == (P, V, ldo)
    if out is None:
        out = tuple(torch.empty(tuple(sh), dtype=torch.float32, device=g.device) for sh in latent_shapes)
    for o, sh in zip(out, latent_shapes):
        assert tuple(o.shape) == tuple(sh) and o.dtype is torch.float32 and o.is_contiguous()
    _check(lib.th_latent_gather_bwd(ctx(g.device), dims, V, H, W, _p(p), P, _p(cams), _p(scale_xy), _p(g), ldo, _p(out[0]),
                                    _p(out[1]), _p(out[2]), _stream()))
    return tuple(out)


# the sizes at which k_latgather_ord.hip takes another path (its LGO_B, LGO_ROUND, LGO_TILE, LGO_LIFT_ROWS): pairs = P * V
LATENT_GATHER_ORDERED_SIZES = dict(batch=64, sort_round=256, sort_tile=2048, lift_rows=256)


def latent_gather_bwd_ordered(latent_shapes, image_hw, pts_world, cams, scale_xy, grad_out, rgb_s=None, out=None,
                              workspace=None):
    """th_latent_gather_bwd_ordered: what latent_gather_bwd computes, with no float atomic and every sum in a fixed order
    (bit-identical from run to run) -> the three latent gradients; with ``rgb_s`` [P,V,4] (latent_gather's second result) also
    the lift's gradients: (g0, g1, g2, g_w [128,3], g_b [128]).  ``out`` (optional, three tensors) is written in full;
    ``workspace`` (optional, uint8) replaces the one allocated here and may hold anything."""
    lib = load_library()
    V, dims = _latent_dims(latent_shapes)
    H, W = (int(x) for x in image_hw)
    p, g = _f32(pts_world).reshape(-1, 3), _f32(grad_out)
    P, ldo = p.shape[0], g.shape[-1]
    assert g.shape == (P, V, ldo)
    if out is None:
        out = tuple(torch.empty(tuple(sh), dtype=torch.float32, device=g.device) for sh in latent_shapes)
    for o, sh in zip(out, latent_shapes):
        assert tuple(o.shape) == tuple(sh) and o.dtype is torch.float32 and o.is_contiguous()
    lift = ()
    if rgb_s is not None:
        rgb_s = _f32(rgb_s)
        assert rgb_s.shape == (P, V, 4)
        lift = (torch.empty((128, 3), dtype=torch.float32, device=g.device),
                torch.empty(128, dtype=torch.float32, device=g.device))
    need = lib.th_latent_gather_bwd_ordered_ws(V, H, W, P)
    ws = _ws(need, g.device) if workspace is None else workspace
    assert ws.dtype is torch.uint8 and ws.is_contiguous() and ws.device == g.device
    _check(lib.th_latent_gather_bwd_ordered(ctx(g.device), dims, V, H, W, _p(p), P, _p(cams), _p(scale_xy), _p(g), ldo,
                                            _p(rgb_s), _p(out[0]), _p(out[1]), _p(out[2]), _p(lift[0] if lift else None),
                                            _p(lift[1] if lift else None), _p(ws), ws.numel(), _stream()))
    return tuple(out) + lift


def composite_bwd(raw, z, ray_d, g_rgb, g_acc, g_depth, white_bkgd=False):
    """th_composite_bwd: the gradients of composite's three outputs -> g_raw [R,S,4]"""
    lib = load_library()
    raw, z, d = _f32(raw), _f32(z), _f32(ray_d).reshape(-1, 3)
    R, S = z.shape
    gr, ga, gd = _f32(g_rgb).reshape(R, 3), _f32(g_acc).reshape(R), _f32(g_depth).reshape(R)
    pts = ThPoints(None, None, _p(d), None, None, None, None, R, S)
    out = torch.empty((R, S, 4), dtype=torch.float32, device=raw.device)
    _check(lib.th_composite_bwd(ctx(raw.device), _p(raw), _p(z), C.byref(pts), int(white_bkgd), _p(gr), _p(ga), _p(gd), _p(out),
                                _stream()))
    return out


def gen_rays(K, R, T, bounds, H, W, device=None, compact=True):
    """Rays of one target camera + box near/far, if_nerf_data_utils.py:11-30, :65-97 (test split of
    sample_ray_h36m :271-283).  K [3,3], R [3,3], T [3,1], bounds [2,3]: float32 numpy / torch (host values).
    compact=True returns the reference's masked ray list {ray_o [R',3], ray_d [R',3], near [R'], far [R'],
    mask_at_box bool [H*W]}; compact=False the dense per-pixel arrays."""
    import numpy as np
    lib = load_library()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)

    def host(a, n):
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        assert a.size == n
        return a

    k, r, t, b = host(K, 9), host(R, 9), host(T, 3), host(bounds, 6)
    n = H * W
    ray_o = torch.empty((n, 3), dtype=torch.float32, device=dev)
    ray_d = torch.empty((n, 3), dtype=torch.float32, device=dev)
    near = torch.empty(n, dtype=torch.float32, device=dev)
    far = torch.empty(n, dtype=torch.float32, device=dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    fp = lambda a: a.ctypes.data_as(c_float_p)
    _check(lib.th_gen_rays(ctx(dev), fp(k), fp(r), fp(t), fp(b), H, W, _p(ray_o), _p(ray_d), _p(near), _p(far), _p(mask),
                           _stream()))
    m = mask.bool()
    if not compact:
        return dict(ray_o=ray_o, ray_d=ray_d, near=near, far=far, mask_at_box=m)
    return dict(ray_o=ray_o[m], ray_d=ray_d[m], near=near[m], far=far[m], mask_at_box=m)


def bound_corners_2d(bounds, K, pose):
    """The eight corners of ``bounds`` [2,3] projected into the camera (K [3,3], pose = [R|T] [3,4]) and rounded
    to integer pixels exactly like if_nerf_data_utils.py:33-53 (get_bound_corners, base_utils.project :178-187,
    np.round(..).astype(int)); the dtype of the inputs is kept, as numpy would."""
    import numpy as np
    bounds, K, pose = np.asarray(bounds), np.asarray(K), np.asarray(pose)
    mn, mx = bounds[0], bounds[1]
    corners = np.array([[mn[0], mn[1], mn[2]], [mn[0], mn[1], mx[2]], [mn[0], mx[1], mn[2]], [mn[0], mx[1], mx[2]],
                        [mx[0], mn[1], mn[2]], [mx[0], mn[1], mx[2]], [mx[0], mx[1], mn[2]], [mx[0], mx[1], mx[2]]])
    xyz = np.dot(corners, pose[:, :3].T) + pose[:, 3:].T
    xyz = np.dot(xyz, K.T)
    xy = xyz[:, :2] / xyz[:, 2:]
    return np.round(xy).astype(int)


def bound_2d_mask(bounds, K, pose, H, W, device=None):
    """th_bound_mask: get_bound_2d_mask (if_nerf_data_utils.py:49-62) -> uint8 [H, W] device tensor."""
    import numpy as np
    lib = load_library()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    c2 = np.ascontiguousarray(bound_corners_2d(bounds, K, pose), dtype=np.int32)
    mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
    _check(lib.th_bound_mask(ctx(dev), c2.ctypes.data_as(C.POINTER(C.c_int32)), H, W, _p(mask), _stream()))
    return mask


def patch_rays(dense, msk, bound_mask, img, draws, subject_ratio, patch_size):
    """th_patch_rays (K18): the train split of sample_ray_patch (if_nerf_data_utils.py:445-499) on the dense arrays of
    ``gen_rays(..., compact=False)``.  ``dense``: {ray_o, ray_d [H*W,3], near, far [H*W], mask_at_box bool / uint8 [H*W]}; ``msk``,
    ``bound_mask`` uint8 [H,W]; ``img`` float32 [H,W,3] or [3,H,W] (read in place through its strides); ``draws`` float64 [N,2] --
    device tensors.  Returns the raw device outputs, the ray rows allocated at their bound N P^2: {patch_masks, patch_masks_sub
    uint8 [N,P,P], target_patches [N,P,P,3], xy_min int32 [N,2], counts int32 [2,N] (candidate pixels, rays per patch), rgb, ray_o,
    ray_d [N P^2,3], near, far [N P^2], sub_mask uint8 [N P^2], select_inds int64 [N P^2]}.  No host wait; sizes outside the
    kernel's limits raise HipError before any launch."""
    lib = load_library()
    H, W = (int(n) for n in msk.shape)
    dev = msk.device
    N, P = int(draws.shape[0]), int(patch_size)
    (ray_o, ray_d, near, far, rm), pix, chan = _dense_ray_inputs(dense, img, H, W)
    assert bound_mask.shape == msk.shape
    assert msk.dtype is torch.uint8 and bound_mask.dtype is torch.uint8 and draws.dtype is torch.float64 and draws.shape[1] == 2
    msk, bound_mask, draws = msk.contiguous(), bound_mask.contiguous(), draws.contiguous()
    rows = max(N * P * P, 1)
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = dict(patch_masks=e((N, P, P), torch.uint8), patch_masks_sub=e((N, P, P), torch.uint8),
               target_patches=e((N, P, P, 3), torch.float32), xy_min=e((N, 2), torch.int32), counts=e((2, N), torch.int32),
               rgb=e((rows, 3), torch.float32), ray_o=e((rows, 3), torch.float32), ray_d=e((rows, 3), torch.float32),
               near=e((rows,), torch.float32), far=e((rows,), torch.float32), sub_mask=e((rows,), torch.uint8),
               select_inds=e((rows,), torch.int64))
    ws = _ws(lib.th_patch_workspace_bytes(H, W), dev)
    _check(lib.th_patch_rays(ctx(dev), _p(ray_o), _p(ray_d), _p(near), _p(far), _p(rm), _p(msk), _p(bound_mask), _p(img), pix, chan,
                             H, W, _p(draws), float(subject_ratio), N, P, *(_p(out[k]) for k in (
                                 "patch_masks", "patch_masks_sub", "target_patches", "xy_min", "counts", "rgb", "ray_o", "ray_d",
                                 "near", "far", "sub_mask", "select_inds")), _p(ws), ws.numel(), _stream()))
    return out


def _dense_ray_inputs(dense, img, H, W):
    """the arguments th_patch_rays, th_ray_sample_train and th_ray_sample_test share: the four dense arrays of ``gen_rays`` and its
    box mask as uint8, and the image's pixel / channel strides"""
    if img.dim() != 3 or img.dtype is not torch.float32:
        raise ValueError(f"img must be float32 [H,W,3] or [3,H,W], got {img.dtype} {tuple(img.shape)}")
    if tuple(img.shape) == (H, W, 3) and (img.stride(0) == W * img.stride(1) or H == 1):
        pix, chan = img.stride(1), img.stride(2)
    elif tuple(img.shape) == (3, H, W) and (img.stride(1) == W * img.stride(2) or H == 1):
        pix, chan = img.stride(2), img.stride(0)
    else:
        raise ValueError(f"img {tuple(img.shape)} with strides {img.stride()}: [H,W,3] or [3,H,W] for H, W = {H}, {W}, its rows "
                         "W pixels apart")
    rm = dense["mask_at_box"]
    rm = (rm.view(torch.uint8) if rm.dtype is torch.bool else rm).contiguous()
    ray_o, ray_d, near, far = (_f32(dense[k]) for k in ("ray_o", "ray_d", "near", "far"))
    assert rm.numel() == H * W and ray_o.numel() == 3 * H * W and ray_d.numel() == 3 * H * W
    assert near.numel() == H * W and far.numel() == H * W
    return (ray_o, ray_d, near, far, rm), pix, chan


def ray_sample_train(dense, msk, bound_mask, img, draws, nrays, body_ratio, face_ratio):
    """th_ray_sample_train (K26): the train split of sample_ray_h36m (if_nerf_data_utils.py:532-598) on the dense arrays of
    ``gen_rays(..., compact=False)``; the arguments of ``patch_rays``, with ``draws`` float64 [4,3,nrays].  Returns the raw device
    outputs, the ray rows allocated at their bound nrays + 4: {rgb, ray_o, ray_d [.,3], near, far [.], coord int64 [.,2], info
    int32 [4] (ray count, iterations, status bits 1 = an iteration added nothing / 2 = unfinished / 4 = a negative class count, the
    last iteration's candidates)}; only the first info[0] rows are written.  No host wait; sizes outside the kernel's limits raise
    HipError before any launch."""
    lib = load_library()
    H, W = (int(n) for n in msk.shape)
    dev, nrays = msk.device, int(nrays)
    arrays, pix, chan = _dense_ray_inputs(dense, img, H, W)
    assert msk.dtype is torch.uint8 and bound_mask.dtype is torch.uint8 and bound_mask.shape == msk.shape
    assert draws.dtype is torch.float64 and tuple(draws.shape) == (4, 3, max(nrays, 0))
    msk, bound_mask, draws = msk.contiguous(), bound_mask.contiguous(), draws.contiguous()
    rows = max(nrays, 0) + 4
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = dict(rgb=e((rows, 3), torch.float32), ray_o=e((rows, 3), torch.float32), ray_d=e((rows, 3), torch.float32),
               near=e((rows,), torch.float32), far=e((rows,), torch.float32), coord=e((rows, 2), torch.int64),
               info=e((4,), torch.int32))
    ws = _ws(lib.th_ray_sample_workspace_bytes(H, W, nrays), dev)
    _check(lib.th_ray_sample_train(ctx(dev), *(_p(a) for a in arrays), _p(msk), _p(bound_mask), _p(img), pix, chan, H, W, _p(draws),
                                   nrays, float(body_ratio), float(face_ratio), *(_p(out[k]) for k in (
                                       "rgb", "ray_o", "ray_d", "near", "far", "coord", "info")), _p(ws), ws.numel(), _stream()))
    return out


def ray_sample_test(dense, img, H, W):
    """th_ray_sample_test (K26): the test split of sample_ray_h36m (if_nerf_data_utils.py:600-612) -- the rows of the dense arrays
    of ``gen_rays(..., compact=False)`` and of ``img`` (float32 [H,W,3] or [3,H,W], read through its strides) where mask_at_box
    holds, in row-major order.  Returns the raw device outputs, the rows allocated at H W: {rgb, ray_o, ray_d [.,3], near, far [.],
    info int32 [4] (info[0] = the count)}; only the first info[0] rows are written.  No host wait."""
    lib = load_library()
    H, W = int(H), int(W)
    dev = img.device
    arrays, pix, chan = _dense_ray_inputs(dense, img, H, W)
    rows = max(H * W, 1)
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = dict(rgb=e((rows, 3), torch.float32), ray_o=e((rows, 3), torch.float32), ray_d=e((rows, 3), torch.float32),
               near=e((rows,), torch.float32), far=e((rows,), torch.float32), info=e((4,), torch.int32))
    ws = _ws(lib.th_ray_sample_workspace_bytes(H, W, 0), dev)
    _check(lib.th_ray_sample_test(ctx(dev), *(_p(a) for a in arrays), _p(img), pix, chan, H, W, *(_p(out[k]) for k in (
        "rgb", "ray_o", "ray_d", "near", "far", "info")), _p(ws), ws.numel(), _stream()))
    return out


def ray_acc(coord, msk):
    """th_ray_acc (K26): get_acc (if_nerf_data_utils.py:635-641).  coord int64 [n,2] = (row, col), msk uint8 [H,W] -- device tensors.
    Returns uint8 [n]: 1 where any pixel of msk is nonzero in the 25 x 25 window centred on the coordinate, clipped to the image.
    No host wait."""
    lib = load_library()
    H, W = (int(n) for n in msk.shape)
    assert coord.dtype is torch.int64 and coord.dim() == 2 and coord.shape[1] == 2 and msk.dtype is torch.uint8
    coord, msk = coord.contiguous(), msk.contiguous()
    n = int(coord.shape[0])
    acc = torch.empty(n, dtype=torch.uint8, device=msk.device)
    _check(lib.th_ray_acc(ctx(msk.device), _p(coord), n, _p(msk), H, W, _p(acc), _stream()))
    return acc


def truncate_select(pts_smpl, centres, sigma):
    """th_truncate_select (K27): cfg.use_truncation's mask_preserve (cross_transformer.py:175-180).  pts_smpl [P,3], centres [N_c,3]
    -> (mask uint8 [P], sel int32 [P'] = the kept indices, ascending, P').  A sample is kept when the fp32 distance to its nearest
    centre -- K4's own -- is below fp32(sigma).  One host read: the count (4 bytes)."""
    lib = load_library()
    p, c = _f32(pts_smpl).reshape(-1, 3), _f32(centres).reshape(-1, 3)
    P, nc = p.shape[0], c.shape[0]
    mask = torch.empty(P, dtype=torch.uint8, device=p.device)
    sel = torch.empty(P, dtype=torch.int32, device=p.device)
    count = torch.empty(1, dtype=torch.int32, device=p.device)
    ws = _ws(lib.th_truncate_select_workspace_bytes(P, nc), p.device)
    _check(lib.th_truncate_select(ctx(p.device), _p(p), P, _p(c), nc, float(sigma), _p(mask), _p(sel), _p(count), _p(ws),
                                  ws.numel(), _stream()))
    n = int(count.item())
    return mask, sel[:n], n


def _truncate_lists(fn, mask, sel):
    assert mask.is_cuda and mask.dtype is torch.uint8 and mask.dim() == 1 and mask.is_contiguous(), f"{fn}: mask uint8 [P]"
    assert sel.dtype is torch.int32 and sel.dim() == 1 and sel.is_contiguous() and sel.device == mask.device, f"{fn}: sel int32 [P']"
    return int(mask.shape[0]), int(sel.shape[0])


def truncate_scatter(rows_kept, mask, sel):
    """th_truncate_scatter (K27): rows_kept [P',4] -> rows [P,4] with rows[sel[j]] = rows_kept[j] and exact zeros where mask is 0
    (raw[:, mask_preserve, :] = raw_preserved on zeros, cross_transformer.py:256-257); mask, sel from ``truncate_select``."""
    lib = load_library()
    P, n = _truncate_lists("truncate_scatter", mask, sel)
    r = _f32(rows_kept)
    assert r.shape == (n, 4), "truncate_scatter: one row of 4 floats per kept sample"
    rows = torch.empty((P, 4), dtype=torch.float32, device=mask.device)
    _check(lib.th_truncate_scatter(ctx(mask.device), _p(r), _p(mask), _p(sel), n, P, 4, _p(rows), _stream()))
    return rows


def truncate_scatter_bwd(g_rows, sel):
    """th_truncate_scatter_bwd (K27): the adjoint of ``truncate_scatter``, g_rows [P,4] -> g_rows[sel] [P',4]."""
    lib = load_library()
    g = _f32(g_rows)
    assert g.dim() == 2 and g.shape[1] == 4 and sel.dtype is torch.int32 and sel.is_contiguous() and sel.device == g.device
    P, n = int(g.shape[0]), int(sel.shape[0])
    out = torch.empty((n, 4), dtype=torch.float32, device=g.device)
    _check(lib.th_truncate_scatter_bwd(ctx(g.device), _p(g), _p(sel), n, P, 4, _p(out), _stream()))
    return out


def set_truncation(sigma, device=None):
    """th_set_truncation (K27): ``sigma`` > 0 = the frame paths of this device (render_rays, eval_sigma_grid, eval_points) zero the
    raw rows of the hull-valid samples whose nearest token centre is sigma or farther away (cfg.use_truncation at inference);
    0 or None = off, the default.  A value already in force costs nothing."""
    sigma = float(sigma or 0.0)
    st = _state(device)
    if st.handle is None and sigma <= 0.0:
        return                                   # (a context is created off)
    if st.truncation != sigma:
        _check(load_library().th_set_truncation(ctx(device), sigma))
        st.truncation = sigma


def set_dparf(knn, n_freq, alpha, device=None):
    """th_set_dparf: cfg.KNN (1..7), the octave count of the network's PE_relative (1..10) and cfg.KNN_DIST_ALPHA (finite, > 0) of
    every later call on this device that runs K4 or its backward (dparf_encode, dparf_encode_bwd, network_forward, the frame
    paths).  A new context has (7, 10, 0.5); values already in force cost nothing.  Another octave count means another fc_0 width:
    the context's MLP weights are dropped with it and the next call that needs them uploads its network's again."""
    want = (int(knn), int(n_freq), float(alpha))
    st = _state(device)
    if st.dparf != want:
        if st.dparf[1] != want[1] and st.owner.get("mlp") is not None:
            # (the weight image of the other width is about to be rewritten: frames queued on other streams may still read it;
            # rare -- another network -- so it simply drains the device, like _sync_weights)
            torch.cuda.synchronize(st.index)
        _check(load_library().th_set_dparf(ctx(device), want[0], want[1], want[2]))
        if st.dparf[1] != want[1]:
            st.owner.pop("mlp", None)
        st.dparf = want


def dparf_in_force(device=None):
    """(knn, n_freq, alpha) that the K4 calls of ``device`` run under: what set_dparf last set, (7, 10, 0.5) before that"""
    return _state(device).dparf


def ssim(a, b):
    """th_ssim: skimage 0.19's structural_similarity(a, b, multichannel=True) as lib/evaluators/if_nerf.py:108 calls it on
    float64 images (7 x 7 uniform window, sample covariance, data_range 2, mean over the window-interior pixels, then over
    the channels), computed in fp64 on the device.  a, b: float32 [H, W, C] device tensors or strided views of larger
    frames (channels contiguous, pixels C floats apart); runs on the current stream and returns a Python float (waits for
    it).  ValueError below 7 x 7, like skimage."""
    if a.dim() != 3 or a.shape != b.shape:
        raise ValueError(f"ssim expects two images of the same [H, W, C] shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    H, W, Cc = (int(n) for n in a.shape)
    if H < 7 or W < 7:
        raise ValueError(f"ssim: a {H} x {W} image is smaller than the 7 x 7 window")
    assert a.is_cuda and b.is_cuda and a.device == b.device, "expected two tensors on the same device"
    assert a.dtype is torch.float32 and b.dtype is torch.float32, "expected float32 images"
    if not (a.stride() == b.stride() and a.stride(2) == 1 and a.stride(1) == Cc and a.stride(0) >= W * Cc):
        a, b = a.contiguous(), b.contiguous()
    lib = load_library()
    ws = _ws(lib.th_ssim_workspace_bytes(H, W, Cc), a.device)
    out = torch.empty(1, dtype=torch.float64, device=a.device)
    _check(lib.th_ssim(ctx(a.device), _p(a), _p(b), H, W, Cc, int(a.stride(0)), _p(out), _p(ws), ws.numel(), _stream()))
    return float(out.item())


LPIPS_CONV_SHAPES = [(64, 3), (64, 64), (128, 64), (128, 128), (256, 128), (256, 256), (256, 256), (512, 256),
                     (512, 512), (512, 512), (512, 512), (512, 512), (512, 512)]    # (COUT, CIN) of VGG16 features[0:30]
LPIPS_TAP_CHANNELS = [64, 128, 256, 512, 512]


def lpips_pack(conv_w, conv_b, lin_w, device=None):
    """th_lpips_pack: the 13 VGG16 conv weights [COUT, CIN, 3, 3] / biases [COUT] and the 5 LPIPS lin weights [1, C, 1, 1]
    -> the packed device image th_lpips reads (a uint8 tensor; the packing runs on the current stream)."""
    assert len(conv_w) == 13 and len(conv_b) == 13 and len(lin_w) == 5
    dev = torch.device(device) if device is not None else conv_w[0].device
    ws = [w.detach().to(dev, torch.float32).contiguous() for w in conv_w]
    bs = [b.detach().to(dev, torch.float32).contiguous() for b in conv_b]
    ls = [w.detach().to(dev, torch.float32).contiguous() for w in lin_w]
    for i, (w, b) in enumerate(zip(ws, bs)):
        co, ci = LPIPS_CONV_SHAPES[i]
        if tuple(w.shape) != (co, ci, 3, 3) or tuple(b.shape) != (co,):
            raise ValueError(f"conv {i}: expected weight {(co, ci, 3, 3)} and bias {(co,)}, got {tuple(w.shape)} and "
                             f"{tuple(b.shape)}")
    for k, w in enumerate(ls):
        if w.numel() != LPIPS_TAP_CHANNELS[k]:
            raise ValueError(f"lin{k}: expected {LPIPS_TAP_CHANNELS[k]} weights, got shape {tuple(w.shape)}")
    lib = load_library()
    packed = torch.empty(int(lib.th_lpips_pack_bytes()), dtype=torch.uint8, device=dev)
    arr13, arr5 = C.c_void_p * 13, C.c_void_p * 5
    _check(lib.th_lpips_pack(ctx(dev), arr13(*[t.data_ptr() for t in ws]), arr13(*[t.data_ptr() for t in bs]),
                             arr5(*[t.data_ptr() for t in ls]), _p(packed), packed.numel(), _stream()))
    torch.cuda.current_stream(dev).synchronize()             # (the sources are temporaries)
    return packed


def lpips(in0, in1, packed):
    """th_lpips: LPIPS (VGG16, v0.1, lpips=True, spatial=False) of in0 vs in1, NCHW float32 device tensors in [-1, 1]
    ([N, 3, H, W] or [3, H, W]), with the image of lpips_pack.  Returns a float64 device tensor [N, 6]: the five tap values
    (relu1_2 .. relu5_3, each already the spatial mean of lin_k((f0 - f1)^2)) and their sum.  Runs on the current stream.
    ValueError below 16 x 16 (the fifth tap would be empty)."""
    if in0.dim() == 3:
        in0, in1 = in0[None], in1[None]
    if in0.dim() != 4 or in0.shape != in1.shape or in0.shape[1] != 3:
        raise ValueError(f"lpips expects two [N, 3, H, W] batches of the same shape, got {tuple(in0.shape)} and "
                         f"{tuple(in1.shape)}")
    N, _, H, W = (int(n) for n in in0.shape)
    if H < 16 or W < 16:
        raise ValueError(f"lpips: a {H} x {W} image is smaller than 16 x 16 (VGG16's fifth tap would be empty)")
    assert in0.is_cuda and in1.is_cuda and in0.device == in1.device == packed.device, "expected tensors on one device"
    a, b = _f32(in0), _f32(in1)
    lib = load_library()
    ws = _ws(lib.th_lpips_workspace_bytes(N, H, W), a.device)
    out = torch.empty((N, 6), dtype=torch.float64, device=a.device)
    _check(lib.th_lpips(ctx(a.device), _p(a), _p(b), N, H, W, _p(packed), _p(out), _p(ws), ws.numel(), _stream()))
    return out


def lpips_pack_bwd(conv_w, device=None):
    """th_lpips_pack_bwd: the 13 VGG16 conv weights [COUT, CIN, 3, 3] (as lpips_pack takes them) -> the packed device image
    of the input-gradient convolutions that th_lpips_bwd reads (a uint8 tensor, about the size of lpips_pack's)."""
    assert len(conv_w) == 13
    dev = torch.device(device) if device is not None else conv_w[0].device
    ws = [w.detach().to(dev, torch.float32).contiguous() for w in conv_w]
    for i, w in enumerate(ws):
        co, ci = LPIPS_CONV_SHAPES[i]
        if tuple(w.shape) != (co, ci, 3, 3):
            raise ValueError(f"conv {i}: expected weight {(co, ci, 3, 3)}, got {tuple(w.shape)}")
    lib = load_library()
    packed = torch.empty(int(lib.th_lpips_bwd_pack_bytes()), dtype=torch.uint8, device=dev)
    arr13 = C.c_void_p * 13
    _check(lib.th_lpips_pack_bwd(ctx(dev), arr13(*[t.data_ptr() for t in ws]), _p(packed), packed.numel(), _stream()))
    torch.cuda.current_stream(dev).synchronize()             # (the sources are temporaries)
    return packed


def _lpips_dims(fn, in0, in1=None):
    if in0.dim() != 4 or in0.shape[1] != 3 or (in1 is not None and in0.shape != in1.shape):
        raise ValueError(f"{fn} expects [N, 3, H, W] batches of one shape, got {tuple(in0.shape)}" +
                         (f" and {tuple(in1.shape)}" if in1 is not None else ""))
    N, _, H, W = (int(n) for n in in0.shape)
    if H < 16 or W < 16:
        raise ValueError(f"{fn}: a {H} x {W} image is smaller than 16 x 16 (VGG16's fifth tap would be empty)")
    return N, H, W


def lpips_train(in0, in1, packed, state=None):
    """th_lpips_train: lpips() -- the same launches, a bit-identical [N, 6] float64 result -- that keeps what the backward
    needs in `state` (a uint8 device tensor of th_lpips_train_state_bytes; allocated when None).  -> (out, state)"""
    N, H, W = _lpips_dims("lpips_train", in0, in1)
    if not (in0.is_cuda and in1.is_cuda):
        raise HipError("lpips_train needs its tensors on an MI355X (there is no CPU path)")
    assert in0.device == in1.device == packed.device, "expected tensors on one device"
    a, b = _f32(in0), _f32(in1)
    lib = load_library()
    nbytes = int(lib.th_lpips_train_state_bytes(N, H, W))
    if state is None:
        state = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
    assert state.dtype is torch.uint8 and state.numel() >= nbytes and state.device == a.device
    out = torch.empty((N, 6), dtype=torch.float64, device=a.device)
    _check(lib.th_lpips_train(ctx(a.device), _p(a), _p(b), N, H, W, _p(packed), _p(out), _p(state), state.numel(), _stream()))
    return out, state


def lpips_bwd(g_out, in0, state, packed, packed_bwd, workspace=None):
    """th_lpips_bwd: the gradient of sum_n g_out[n] * lpips_train(in0, in1)[n, 5] with respect to in0 -> float32 [N, 3, H, W].
    g_out: [N] (any float dtype; float64 on the device); state: lpips_train's, of the same in0."""
    N, H, W = _lpips_dims("lpips_bwd", in0)
    assert in0.is_cuda and in0.device == state.device == packed.device == packed_bwd.device, "expected tensors on one device"
    a = _f32(in0)
    g = g_out.detach().reshape(-1).to(a.device, torch.float64).contiguous()
    if g.numel() != N:
        raise ValueError(f"lpips_bwd: g_out has {g.numel()} elements for a batch of {N}")
    lib = load_library()
    nbytes = int(lib.th_lpips_bwd_workspace_bytes(N, H, W))
    ws = workspace if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=a.device)
    assert ws.dtype is torch.uint8 and ws.numel() >= nbytes and ws.device == a.device
    out = torch.empty((N, 3, H, W), dtype=torch.float32, device=a.device)
    _check(lib.th_lpips_bwd(ctx(a.device), _p(g), _p(a), N, H, W, _p(packed), _p(packed_bwd), _p(state), state.numel(), _p(out),
                            _p(ws), ws.numel(), _stream()))
    return out


def lpips_dgrad(layer, g, packed_bwd, gate=None):
    """th_lpips_dgrad: the input gradient of VGG16 conv `layer` (0..12) on its own.  g: float32 NHWC [Z, H, W, COUT] ->
    NHWC [Z, H, W, CIN], zeroed where `gate` (same shape) is <= 0; layer 0: NCHW [Z, 3, H, W] times 1 / scale[c]."""
    co, ci = LPIPS_CONV_SHAPES[layer]
    g = _f32(g)
    Z, H, W, Cg = (int(n) for n in g.shape)
    if Cg != co:
        raise ValueError(f"lpips_dgrad: layer {layer} takes {co} channels, got {Cg}")
    out = torch.empty((Z, 3, H, W) if layer == 0 else (Z, H, W, ci), dtype=torch.float32, device=g.device)
    if gate is not None:
        gate = _f32(gate)
        assert tuple(gate.shape) == tuple(out.shape)
    _check(load_library().th_lpips_dgrad(ctx(g.device), layer, _p(g), _p(gate), Z, H, W, _p(packed_bwd), _p(out), _stream()))
    return out


def lpips_pool_bwd(g, y):
    """th_lpips_pool_bwd: backward of the 2 x 2 / stride 2 max pool.  g: NHWC [Z, H // 2, W // 2, C], y: the pooled map's
    source NHWC [Z, H, W, C] -> [Z, H, W, C]."""
    g, y = _f32(g), _f32(y)
    Z, H, W, Cc = (int(n) for n in y.shape)
    assert tuple(g.shape) == (Z, H // 2, W // 2, Cc)
    out = torch.empty_like(y)
    _check(load_library().th_lpips_pool_bwd(ctx(y.device), _p(g), _p(y), Z, H, W, Cc, _p(out), _stream()))
    return out


def lpips_head_bwd(f0, f1, lin, g_out, g=None, gate=False):
    """th_lpips_head_bwd: f0, f1 float32 [N, hw, C], lin [C], g_out float64 [N] -> [N, hw, C]: g (when given, in place) plus
    the fp32-rounded derivative of the head with respect to f0; gate=True zeroes it where f0 <= 0."""
    f0, f1, lin = _f32(f0), _f32(f1), _f32(lin).reshape(-1)
    N, hw, Cc = (int(n) for n in f0.shape)
    assert f1.shape == f0.shape and lin.numel() == Cc
    go = g_out.detach().reshape(-1).to(f0.device, torch.float64).contiguous()
    assert go.numel() == N
    acc = g is not None
    if acc:
        assert g.dtype is torch.float32 and g.is_contiguous() and g.shape == f0.shape
    else:
        g = torch.empty_like(f0)
    _check(load_library().th_lpips_head_bwd(ctx(f0.device), _p(f0), _p(f1), N, hw, Cc, _p(lin), _p(go), int(acc), int(gate),
                                            _p(g), _stream()))
    return g


def marching_cubes(cube, iso, scale=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), x_range=None):
    """th_marching_cubes_*: mcubes.marching_cubes(cube, iso) on the device (if_mesh_renderer.py:103) with the
    index -> world transform of :106-108 applied (vertex = index * scale + origin, float64).
    cube: [X,Y,Z] fp32 device tensor.  -> (vertices float64 [nv,3], triangles int32 [nt,3]) device tensors.
    x_range=(x0, x1): only the grid slab x0 <= x < x1 is emitted (multi-GPU z-slab style sharding); returns
    (vertices, triangles, (v0, v1), (t0, t1)) where the slab filled rows [v0, v1) / [t0, t1) of the full arrays."""
    lib = load_library()
    c = _f32(cube)
    assert c.dim() == 3
    X, Y, Z = c.shape
    dev = c.device
    ws = _ws(lib.th_marching_cubes_workspace_bytes(X, Y, Z), dev)
    counts = (C.c_int64 * 2)()
    _check(lib.th_marching_cubes_count(ctx(dev), _p(c), X, Y, Z, float(iso), _p(ws), ws.numel(), counts, _stream()))
    nv, nt = int(counts[0]), int(counts[1])
    verts = torch.zeros((nv, 3), dtype=torch.float64, device=dev)
    tris = torch.zeros((nt, 3), dtype=torch.int32, device=dev)
    sc = (C.c_double * 3)(*[float(v) for v in scale])
    og = (C.c_double * 3)(*[float(v) for v in origin])
    x0, x1 = (0, X) if x_range is None else (int(x_range[0]), int(x_range[1]))
    if nv > 0:
        _check(lib.th_marching_cubes_emit(ctx(dev), _p(c), X, Y, Z, float(iso), _p(ws), x0, x1, sc, og,
                                          _p(verts), _p(tris) if nt > 0 else _p(verts), _stream()))
    if x_range is None:
        return verts, tris
    a, b = (C.c_int64 * 2)(), (C.c_int64 * 2)()
    _check(lib.th_marching_cubes_range(ctx(dev), _p(ws), X, Y, Z, max(x0, 0), a, _stream()))
    _check(lib.th_marching_cubes_range(ctx(dev), _p(ws), X, Y, Z, min(x1, X), b, _stream()))
    return verts, tris, (int(a[0]), int(b[0])), (int(a[1]), int(b[1]))


class SmplModel:
    """Device copy of the SMPL model arrays (the fields lib/utils/SMPL.py:83-89 reads), float64."""

    def __init__(self, arrays, device=None):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        f64 = lambda k: torch.as_tensor(arrays[k], dtype=torch.float64).contiguous().to(dev)
        self.v_template, self.shapedirs, self.posedirs = f64("v_template"), f64("shapedirs"), f64("posedirs")
        self.J_regressor, self.weights = f64("J_regressor"), f64("weights")
        self.parent = torch.as_tensor(arrays["parent"], dtype=torch.int32).contiguous().to(dev)
        self.nv = self.v_template.shape[0]
        assert self.shapedirs.shape == (self.nv, 3, 10) and self.posedirs.shape == (self.nv, 3, 207)
        assert self.J_regressor.shape == (24, self.nv) and self.weights.shape == (self.nv, 24)
        self.c = ThSmplModel(_p(self.v_template), _p(self.shapedirs), _p(self.posedirs), _p(self.J_regressor),
                             _p(self.weights), _p(self.parent), self.nv)

    def __call__(self, pose, beta):
        """SMPL.__call__ (lib/utils/SMPL.py:107-186): pose = 72 axis-angle values or [24,3,3] rotation matrices;
        beta [10].  -> (v [nv,3], joints [24,3], T [nv,4,4]) float64 device tensors."""
        lib = load_library()
        dev = self.v_template.device
        p = torch.as_tensor(pose, dtype=torch.float32).contiguous().to(dev)
        b = torch.as_tensor(beta, dtype=torch.float64).reshape(10).contiguous().to(dev)
        is_rot = tuple(p.shape) == (24, 3, 3)
        assert is_rot or p.numel() == 72, "Unsupported Pose Inputs"
        v = torch.empty((self.nv, 3), dtype=torch.float64, device=dev)
        j = torch.empty((24, 3), dtype=torch.float64, device=dev)
        T = torch.empty((self.nv, 4, 4), dtype=torch.float64, device=dev)
        ws = _ws(lib.th_smpl_workspace_bytes(self.nv), dev)
        _check(lib.th_smpl_lbs(ctx(dev), C.byref(self.c), None if is_rot else _p(p), _p(p) if is_rot else None, _p(b),
                               _p(v), _p(j), _p(T), _p(ws), ws.numel(), _stream()))
        return v, j, T


def view_embed(ray_d, view_res=4):
    lib = load_library()
    d = _f32(ray_d).reshape(-1, 3)
    out = torch.empty((d.shape[0], 3 + 6 * view_res), dtype=torch.float32, device=d.device)
    _check(lib.th_view_embed(ctx(d.device), _p(d), d.shape[0], view_res, _p(out), _stream()))
    return out


class Frame:
    """Per-frame constants of the per-sample stage (th_frame) + owners."""

    def __init__(self, verts_world, Rh, Th, cams, scale_xy, pixel_map_nhwc, tokens, centres, rot,
                 hull_thresh=0.1, small_frame_rays=2400):
        self.verts = _f32(verts_world).reshape(-1, 3)
        self.Rh, self.Th = _f32(Rh).reshape(9), _f32(Th).reshape(3)
        self.cams, self.scale = cams, scale_xy
        self.map = pixel_map_nhwc
        self.centres, self.rot = _f32(centres).reshape(-1, 3), _f32(rot).reshape(-1, 9)
        self.tokens = _f32(tokens) if tokens is not None else None       # None: set_tokens() before the frame is rendered
        # set by Renderer.prepare_frame: ``rebuild()`` -> the same constants again (range guard), ``stem_flag`` (device bool: the
        # stem latents received from another rank were not finite), ``finish_tokens()`` (TransHE of a frame built without it)
        self.rebuild = self.stem_flag = self.finish_tokens = None
        V, H, W, Cc = pixel_map_nhwc.shape
        assert Cc in (384, 260) or isinstance(pixel_map_nhwc, SplitMap), \
            "pixel map must be the full (384) or the compact (260 interleaved / SplitMap) channels-last map"
        src = getattr(pixel_map_nhwc, "source", None)
        self.c = ThFrame(_p(self.verts), self.verts.shape[0], _p(self.Rh), _p(self.Th), _p(self.cams), _p(self.scale),
                         _p(self.map), V, H, W, Cc, _p(self.tokens), _p(self.centres), _p(self.rot),
                         self.centres.shape[0], hull_thresh, small_frame_rays,
                         C.cast(C.pointer(src[0]), C.c_void_p).value if src is not None else None,
                         _p(getattr(pixel_map_nhwc, "fold", None)))

    def set_tokens(self, tokens):
        """TransHE output [V, N_c, 192] of a frame that was built without it (render_pregather runs beside TransHE)"""
        self.tokens = _f32(tokens)
        assert self.tokens.shape[1] == self.centres.shape[0]
        self.c.tokens = self.tokens.data_ptr()


def _cached_ws(nbytes, device, slot=0):
    """Render workspace, grown on demand.  ``slot`` selects one of several independent workspaces (the frame
    pipeline of Renderer.render_sequence runs the hull stage of frame i+1 while frame i is still shading)."""
    cache = _state(device).workspaces
    cur = cache.get(slot)
    if cur is None or cur.numel() < nbytes:
        cache[slot] = None
        cur = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        cache[slot] = cur
    return cur


def _shade_pool(frame_c, n_valid, with_pregather, device, slot=None):
    """The context's shading pool (include/transhuman_hip.h: th_shade_pool_bytes), ONE per device, grown on demand to what
    ``n_valid`` valid samples need in the context's current mode.  Growth allocates on the current stream; the old pool
    goes back to torch's allocator, which hands it out again only behind the work already queued on it."""
    need = int(load_library().th_shade_pool_bytes(ctx(device), C.byref(frame_c), int(n_valid), int(with_pregather)))
    # (slot: a frame pipeline that forms the NEXT frame's records while this frame shades gives every frame in flight a pool of
    # its own -- Renderer.render_sequence; None: the context's one shared pool)
    cache, key = _state(device).pools, None if slot is None else int(slot)
    cur = cache.get(key)
    if cur is None or cur.numel() < need:
        cache[key] = None
        # (headroom: frames of a sequence differ by a few per cent; a pool that grows every other frame would thrash)
        cur = torch.empty(int(need * 1.0625) + 4096, dtype=torch.uint8, device=device)
        cache[key] = cur
    cur.record_stream(torch.cuda.current_stream(device))
    return cur


def shared_pool(device=None):
    """the context's shared shading pool as it is cached now (a uint8 device tensor), or None"""
    return _state(device).pools.get(None)


def _prepass_counts(ws, device):
    """(hit_rays, unmasked, n_valid) of the prepass pending in workspace ``ws`` (host wait), or None"""
    out = (C.c_int64 * 3)()
    rc = load_library().th_render_prepass_wait(ctx(device), _p(ws), out)
    if rc == 1:
        return None
    _check(rc)
    return int(out[0]), int(out[1]), int(out[2])


def drop_workspaces(device=None):
    """Forget the cached render workspaces and the shading pool (GBs at full frame size) -- e.g. between unrelated
    workloads of one process; pending prepasses of those workspaces are cancelled."""
    lib = load_library()
    for st in (set(_states.values()) if device is None else [_state(device)]):
        st.pools.clear()
        st.workspaces.clear()
    try:
        _check(lib.th_render_prepass_cancel(ctx(device)))
    except HipError:
        pass


def render_prepass(points, verts_world, V, hull_thresh=0.1, small_frame_rays=2400, n_clusters=0, slot=0):
    """th_render_prepass: queue the ray-only front of render_rays (hull mask, compaction, ...) before the
    per-frame constants exist.  The following render_rays on the same `points` picks it up (and shades in the
    workspace ``slot`` the prepass wrote)."""
    lib = load_library()
    v = _f32(verts_world).reshape(-1, 3)
    dev = v.device
    f = ThFrame()
    f.verts_world, f.n_verts, f.V = v.data_ptr(), v.shape[0], V
    f.hull_thresh, f.small_frame_rays, f.map_channels = hull_thresh, small_frame_rays, 384
    f.n_clusters = n_clusters                  # (sizes the workspace exactly like the frame that follows)
    ws = _cached_ws(lib.th_render_workspace_bytes(C.byref(f), points.R, points.S), dev, slot)
    points._prepass_keep = (v, ws)
    points._prepass_nc = int(n_clusters)
    _check(lib.th_render_prepass(ctx(dev), C.byref(f), C.byref(points.c), _p(ws), ws.numel(), _stream()))
    points._prepass_pending = True          # only THIS Points object (it keeps the ray tensors alive) may consume it


def render_predemand(points, cams, scale_xy, V, H, W, verts_paint=None):
    """th_render_predemand: behind the pending render_prepass of ``points`` (on the current stream, which is ordered behind it),
    mark the map texels its valid samples -- and the ``verts_paint`` [n,3] vertices, if given -- read in the V views.  -> the demand
    buffer (device uint8 tensor) for upsample_concat_split(demand=...) / map_fold, or None (no pending prepass, or a map
    width that is not a multiple of 64)."""
    if not points._prepass_pending or int(W) % 64 != 0 or V > 3:
        return None
    lib = load_library()
    v, ws = points._prepass_keep
    dev = v.device
    f = ThFrame()
    f.verts_world, f.n_verts, f.V, f.H, f.W = v.data_ptr(), v.shape[0], int(V), int(H), int(W)
    f.cams, f.scale_xy = cams.data_ptr(), scale_xy.data_ptr()
    f.n_clusters, f.map_channels = points._prepass_nc, 384
    vp = _f32(verts_paint).reshape(-1, 3) if verts_paint is not None else None
    nb = int(lib.th_map_demand_bytes(int(V), int(H), int(W)))
    demand = torch.empty(nb, dtype=torch.uint8, device=dev)
    rc = lib.th_render_predemand(ctx(dev), C.byref(f), C.byref(points.c), _p(ws), ws.numel(), _p(vp), vp.shape[0] if vp is not None else 0,
                                 _p(demand), nb, _stream())
    if rc == 1:
        return None
    _check(rc)
    demand._keep = (vp, cams, scale_xy)
    return demand


def render_pregrid(frame, points):
    """th_render_pregrid: the candidate grid of K4's 7-neighbour search for the frame's token centres, into the workspace of
    the pending render_prepass of ``points`` -- on the current stream (the one that produced the centres)."""
    if not points._prepass_pending:
        return
    _, ws = points._prepass_keep
    _check(load_library().th_render_pregrid(ctx(frame.verts.device), C.byref(frame.c), C.byref(points.c), _p(ws), ws.numel(),
                                            _stream()))


def render_pregather(net, frame, points, slot=0, early=False, pool_slot=None):
    """th_render_pregather: behind a render_prepass of the same ``points`` / workspace ``slot``, queue the pixel-feature
    gather and the neighbour records of the first chunks -- ``frame`` may still lack its tokens (Frame(tokens=None)),
    so TransHE can run on another stream meanwhile.  ``early=True`` (th_render_pregather_early): the caller has made the
    current stream wait for this frame's front BEFORE it queued the previous frame's render_rays, so the neighbour
    records may start as soon as that frame's per-sample stage is done, beside its compositing."""
    if not points._prepass_pending:
        return
    lib = load_library()
    _sync_weights(net, "mlp")
    dev = frame.verts.device
    _, ws = points._prepass_keep
    cnt = _prepass_counts(ws, dev)
    if cnt is None:
        return
    pool = _shade_pool(frame.c, cnt[2], True, dev, pool_slot)
    points._pregathered = True
    fn = lib.th_render_pregather_early if early else lib.th_render_pregather
    _check(fn(ctx(dev), C.byref(frame.c), C.byref(points.c), _p(ws), ws.numel(), _p(pool), pool.numel(), _stream()))


def render_rays(net, frame, points, white_bkgd=False, defer_guard=False, small_frame_rays=None, pool_slot=None):
    """th_render_rays: rays -> (rgb [R,3], acc [R], depth [R], stats).
    Range guard: the frame's snapshot of the split-arithmetic maxima is read back after the call (a host wait for
    the frame) and, if a tensor left the resolvable range, the frame is rendered again on the fp32 path.
    ``defer_guard=True`` returns a fifth value, a callable ``check() -> bool`` (True = clean), instead: a frame
    pipeline calls it after queuing the next frame so the host never idles the device.
    ``small_frame_rays``: the R' threshold of if_clight_renderer.py:551 for THIS call (applied to a copy of the
    frame descriptor; None = the frame's own value)."""
    lib = load_library()
    _sync_weights(net, "mlp")
    dev = frame.verts.device
    R = points.R
    rgb = torch.empty((R, 3), dtype=torch.float32, device=dev)
    acc = torch.empty(R, dtype=torch.float32, device=dev)
    dep = torch.empty(R, dtype=torch.float32, device=dev)
    if R == 0:                                   # empty ray list: nothing to launch (zero-size tensors have no address)
        st0 = dict(hit_rays=0, valid_samples=0, unmasked=0)
        return (rgb, acc, dep, st0, lambda: True) if defer_guard else (rgb, acc, dep, st0)
    fc = frame.c
    if small_frame_rays is not None and int(small_frame_rays) != fc.small_frame_rays:
        fc = ThFrame.from_buffer_copy(frame.c)
        fc.small_frame_rays = int(small_frame_rays)
    need = lib.th_render_workspace_bytes(C.byref(fc), R, points.S)
    n_bound, pre = R * points.S, False
    if points._prepass_pending and points._prepass_keep[1].numel() >= need:
        points._prepass_pending = False
        ws = points._prepass_keep[1]                        # the workspace its prepass ran in
        cnt = _prepass_counts(ws, dev)                      # (on the host long ago in a frame pipeline)
        if cnt is not None:
            n_bound, pre = cnt[2], points._pregathered
    else:
        ws = _cached_ws(need, dev)
        _check(lib.th_render_prepass_drop(ctx(dev), _p(ws)))  # a token queued there for other (possibly freed) rays
    points._pregathered = False
    stats, st = (C.c_int64 * 4)(), {}

    def shade(fr, i):                            # try i on frame ``fr`` -> range-guard slot; the statistics into ``st``
        nonlocal fc, n_bound, pre
        if i > 0:
            if fr is not frame:                  # rebuilt (the guard switched the stem / TransHE): this call's R' threshold again
                keep_sfr, fc = fc.small_frame_rays, ThFrame.from_buffer_copy(fr.c)
                fc.small_frame_rays = keep_sfr
            _check(lib.th_render_prepass_drop(ctx(dev), _p(ws)))
            n_bound, pre = st["valid_samples"], False      # (the guard may have changed the mode: other row formats)
        # the shading pool: sized from the valid-sample count when a prepass (or an earlier try) has put it on the host, else
        # for the chunk buffers only (the count bounds the chunk, not the pool)
        pool = _shade_pool(fc, n_bound, pre, dev, pool_slot)
        _check(lib.th_render_rays(ctx(dev), C.byref(fc), C.byref(points.c), _p(rgb), _p(acc), _p(dep), int(white_bkgd),
                                  _p(ws), ws.numel(), _p(pool), pool.numel(), stats, _stream()))
        st.update(hit_rays=stats[0], valid_samples=stats[1], unmasked=stats[3])
        return int(stats[2])
    if defer_guard:
        slot = shade(frame, 0)
        return rgb, acc, dep, st, (lambda: _guard(dev, slot))
    _guarded(dev, shade, 4, frame, check_last=False)
    return rgb, acc, dep, st


def _eval_point_mode(net, frame, pts, dirs, rgb):
    """the body of eval_sigma_grid (``rgb`` False: out [P]) and eval_points (True: out [P,4])"""
    lib = load_library()
    _sync_weights(net, "mlp")
    p = _f32(pts).reshape(-1, 3)
    P = p.shape[0]
    d = None if dirs is None else _f32(dirs).reshape(-1, 3)
    assert d is None or (d.shape[0] == P and d.device == p.device), "one direction per point, on the points' device"
    out = torch.empty((P, 4) if rgb else P, dtype=torch.float32, device=p.device)
    if P == 0:
        return out, dict(valid_samples=0)
    ws = _cached_ws(lib.th_sigma_grid_workspace_bytes(C.byref(frame.c), P), p.device)
    stats = (C.c_int64 * 4)()

    def launch(fr, _i):
        pool = _shade_pool(fr.c, P, False, p.device)           # (per try: the guard may have changed the mode)
        fn, head = (lib.th_eval_points, (_p(p), _p(d), P)) if rgb else (lib.th_eval_sigma_grid, (_p(p), P))
        _check(fn(ctx(p.device), C.byref(fr.c), *head, _p(out), _p(ws), ws.numel(), _p(pool), pool.numel(), stats, _stream()))
        return int(stats[2])
    _guarded(p.device, launch, 3, frame)
    return out, dict(valid_samples=stats[1])


def eval_sigma_grid(net, frame, pts):
    return _eval_point_mode(net, frame, pts, None, False)


def eval_points(net, frame, pts, dirs=None):
    """th_eval_points: the radiance field at arbitrary world-space points.  pts [P,3], dirs [P,3] viewing directions (normalised
    on the device) or None (the zero embedding rows of if_mesh_renderer.py:62) -> (raw fp32 [P,4] = rgb logits + sigma_raw, stats).
    Rows outside the hull are exactly 0; inside, sigma everywhere and the RGB logits where sigma > 0 (0 elsewhere).  Same guard
    and retry as eval_sigma_grid."""
    return _eval_point_mode(net, frame, pts, dirs, True)


def set_tok_gather(on, device=None):
    """Token-branch hand-over K4 -> K6 on the fused path: True (default) = neighbour records, the fused kernel blends the
    rows of the per-frame token table on the matrix pipe; False = K4 blends them in fp32 (3.3 KB per sample through HBM;
    a ray shard then equals the whole frame bit for bit instead of to fp32 rounding)."""
    _check(load_library().th_set_tok_gather(ctx(device), 1 if on else 0))


def _asked(device, name, default):
    """what set_<name> last chose on this device, else ``default`` (nothing set anywhere: no CUDA call on a host without one)"""
    if all(getattr(st, name) is None for st in _states.values()):
        return default
    v = getattr(_state(device), name)
    return default if v is None else v


def tex_rows_enabled(device=None):
    """Whether new frames of this device's context take the texel hand-over (include/transhuman_hip.h: th_set_tex_rows); it
    applies to the fused path on frames with a split map (Renderer.prepare_frame's default)."""
    return _asked(device, "tex_rows", os.environ.get("TH_ROWS_TEX", "1")[:1] != "0")


def mlp_is_fused(device=None):
    """the fused fp16-split kernel shades this device's frames (mode 1 requested and the range guard has not switched it off)"""
    st = _state(device)
    return st.mode["mlp"] in (None, 1) and not st.fallback["mlp"]


def set_tex_rows(on, device=None):
    """Pixel-feature hand-over K5 -> K6 on the fused path (split map): True (default) = texel lists per tile, the fused kernel
    copies the distinct texels into LDS and blends them itself (same operand bits, 160 B instead of 3.3 KB per sample through
    HBM); False = K5 writes the rows.  The shading pool is sized per mode (cached pools are re-made on demand)."""
    _check(load_library().th_set_tex_rows(ctx(device), 1 if on else 0))
    _state(device).tex_rows = bool(on)


def set_mlp_mode(mode, device=None):
    """1 = fused fp16-split MFMA kernel (default), 0 = layer-by-layer fp32 MFMA GEMMs."""
    _restore(_state(device), "mlp", int(mode))


def set_fused_waves(waves, device=None):
    """Form of the fused MLP kernel on the frame-level path: 8 = two waves per SIMD (512-thread workgroups, default), 4 = the
    256-thread form of rounds 2-5."""
    _check(load_library().th_set_fused_waves(ctx(device), int(waves)))
    _state(device).fused_waves = int(waves)


def fused_waves(device=None):
    """what set_fused_waves last chose on this device (default: TH_FUSED_WAVES, else 8)"""
    return _asked(device, "fused_waves", 4 if os.environ.get("TH_FUSED_WAVES", "8")[:1] == "4" else 8)


def set_chunk_samples(n):
    """Samples per pass of the per-sample stage (default 524288; results are invariant to it)."""
    _check(load_library().th_set_chunk_samples(int(n)))


PROF_PHASES = ("hull", "dparf", "gather", "mlp", "composite", "vit", "fold", "_7")


def profile_enable(on=True, device=None):
    _check(load_library().th_profile_enable(ctx(device), int(on)))


def profile_read(device=None):
    """-> {phase: (milliseconds, launches)} accumulated since the last read."""
    ms = (C.c_double * 8)()
    cnt = (C.c_int64 * 8)()
    _check(load_library().th_profile_read(ctx(device), ms, cnt))
    return {PROF_PHASES[i]: (ms[i], cnt[i]) for i in range(7)}


def clock_probe(out):
    """th_clock_probe: queue the shader-clock probe on the current stream; ``out`` = int64 device tensor of >= 3 words
    (ticks, 10 ns units, scratch).  GHz = out[0] / (10 * out[1]) once the stream has passed it."""
    assert out.dtype == torch.int64 and out.numel() >= 3 and out.is_cuda
    _check(load_library().th_clock_probe(ctx(out.device), _p(out), _stream()))


def fused_cycles(counters, device=None):
    """th_fused_cycles: cycle accounting of the fused MLP kernel into ``counters`` (64 zeroed int64 words on the device), or None to
    switch it off.  [0] sampled tiles, [1..61] shader cycles per phase, [62] / [63] shader cycles / 100 MHz ticks per tile."""
    if counters is not None:
        assert counters.dtype == torch.int64 and counters.numel() >= 64 and counters.is_cuda
        device = counters.device
    _check(load_library().th_fused_cycles(ctx(device), _p(counters) if counters is not None else None))


def host_wait_read(device=None):
    """th_host_wait_read: host ms spent in the blocking waits of the entry points since the last call (reads and clears)"""
    ms = C.c_double()
    _check(load_library().th_host_wait_read(ctx(device), C.byref(ms)))
    return float(ms.value)


def set_vit_mode(mode, device=None):
    """th_set_vit_mode: 0 = TransHE's dense layers on the fp32 MFMA GEMMs, 1 (default) = fp16-split arithmetic."""
    _restore(_state(device), "vit", int(mode))
