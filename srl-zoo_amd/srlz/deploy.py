"""Deployment encoder: camera frames to states in four launches.

    enc = StateEncoder(model, max_batch=32, frame_layout="nhwc")      # SRLModules / SRLModulesSplit / a bare CustomCNN, CNNAutoEncoder, CNNVAE
    enc = StateEncoder.from_log_folder("logs/<dataset>/<experiment>/")  # via SRL4robotics.loadSavedModel
    states = enc(frames)        # uint8 [N,H,W,C] or [H,W,C] ("nhwc"), or [N,C,W,H] / [C,W,H] ("planar"); numpy or device tensor -> [N,S] / [S]
    states = enc.numpy(frames)  # the same through a pinned buffer, one synchronisation
    enc.refresh()               # re-read weights and running statistics after more training
    enc.route                   # "blocks" or "model"

What the RL side of the toolbox does with a trained model is `model.getStates(obs)` on one preprocessed camera frame per environment
step, or on n_envs of them.  `getStates` runs the training kernels in eval mode: about ten launches, three autograd nodes per block, and
every raw convolution output written and read back.  In eval mode the BatchNorm statistics are known before the launch, so route
"blocks" runs each encoder block (models/models.py:47-63) as ONE launch of csrc/infer.hip — convolution, affine, ReLU and MaxPool, the raw
convolution output never stored — and the state head on the existing srlz_linear_fwd.  The frames stay bytes: the first block
normalises them through the table of srlz_normalize_lut and reads either byte layout by strides.

The layout is stated by the caller and never guessed from a shape (the rule of BaseLearner.frame_layout).

Route "model" is the model's own getStates under no_grad in eval mode, every module's mode restored: the models without a conv encoder
(mlp, linear, the triplet EmbeddingNet) and calls of more than max_batch frames.  Nothing is rejected, nothing is approximated.

A "blocks" call allocates no device memory, builds no autograd graph, touches neither the running statistics nor num_batches_tracked, the
model's mode or torch's RNG, and runs on the current stream.  The states it returns are a view of the encoder's own buffer: they are
overwritten by the next call (clone them to keep them), and one encoder serves one stream at a time.

The way back — FrameDecoder, states to camera frames in six launches, and reconstruct(encoder, decoder, frames) — is the second half
of this file.
"""
import numpy as np
import torch

from . import _cabi as C
from . import ops

LAYOUTS = ("nhwc", "planar")
ROUTE_BLOCKS, ROUTE_MODEL = "blocks", "model"


def _core(model):
    """The network behind a wrapper: SRL4robotics.model -> SRLModules(.Split).model -> the encoder class."""
    from models.modules import SRLModules, SRLModulesSplit
    if not isinstance(model, torch.nn.Module) and isinstance(getattr(model, "model", None), torch.nn.Module):
        model = model.model  # a learner
    owner = model
    if isinstance(model, (SRLModules, SRLModulesSplit)):
        model = model.model
    return owner, model


def encoder_parts(model):
    """(conv stack, state head) of a model whose getStates is conv encoder + one Linear, else None.
    The head: encoder_fc (AE, autoencoders.py:107-108), encoder_fc1 = mu (VAE, vae.py:52 with models.py:131-139), fc (CustomCNN,
    models.py:209-212).  The dense auto-encoders own a conv stack too (they inherit it) but never run it: chosen by class."""
    from models.models import CustomCNN
    from models.autoencoders import CNNAutoEncoder
    from models.vae import CNNVAE
    _, core = _core(model)
    if isinstance(core, CNNAutoEncoder):
        return core.encoder_conv, core.encoder_fc[0]
    if isinstance(core, CNNVAE):
        return core.encoder_conv, core.encoder_fc1
    if isinstance(core, CustomCNN):
        return core.conv_layers, core.fc
    return None


def route_for(model):
    """The route a StateEncoder of `model` takes for calls within max_batch (host only: no GPU is asked for)."""
    return ROUTE_BLOCKS if encoder_parts(model) is not None else ROUTE_MODEL


def check_layout(frame_layout):
    if frame_layout not in LAYOUTS:
        raise ValueError("frame_layout must be 'nhwc' or 'planar', got %r" % (frame_layout,))
    return frame_layout


def check_frames(frames, frame_layout, channels, frame_size=None):
    """Validate a call's frames against the stated layout: uint8, [N,H,W,C] / [H,W,C] ("nhwc") or [N,C,W,H] / [C,W,H] ("planar"),
    `channels` channels, frame_size = (H, W) when given.  Returns (n, single): frames in the call, whether one bare frame came in."""
    check_layout(frame_layout)
    if not isinstance(frames, (np.ndarray, torch.Tensor)):
        raise ValueError("frames must be a numpy array or a torch tensor, got %s" % type(frames).__name__)
    if frames.dtype != (np.uint8 if isinstance(frames, np.ndarray) else torch.uint8):
        raise ValueError("frames must be uint8 camera bytes (got %s): the encoder normalises them itself" % (frames.dtype,))
    shape = tuple(frames.shape)
    if len(shape) not in (3, 4):
        raise ValueError("frames must be [N,H,W,C] or [H,W,C] ('nhwc') / [N,C,W,H] or [C,W,H] ('planar'), got shape %s" % (shape,))
    single = len(shape) == 3
    full = ((1,) + shape) if single else shape
    if frame_layout == "nhwc":
        n, h, w, c = full
    else:
        n, c, w, h = full
    if c != channels:
        raise ValueError("frames of layout %r with shape %s carry %d channels, the model takes %d" % (frame_layout, shape, c, channels))
    if frame_size is not None and (h, w) != tuple(frame_size):
        raise ValueError("frames are %d x %d (H x W), the encoder was built for %d x %d" % ((h, w) + tuple(frame_size)))
    if n < 1:
        raise ValueError("no frame in the call")
    return n, single


class StateEncoder(object):
    def __init__(self, model, max_batch=32, frame_layout="nhwc", frame_size=(224, 224), route=None):
        """model: SRLModules / SRLModulesSplit / a bare CustomCNN, CNNAutoEncoder, CNNVAE (or any model with getStates: route "model").
        frame_size: (H, W) of the camera frames.  route="model" forces the fallback for every call (tools/kb_deploy.py measures the
        two routes side by side); None picks by model class."""
        self.frame_layout = check_layout(frame_layout)
        if route not in (None, ROUTE_MODEL):
            raise ValueError("route must be None or 'model', got %r" % (route,))
        if int(max_batch) < 1:
            raise ValueError("max_batch must be at least 1, got %r" % (max_batch,))
        from models.learner import _requireGpu
        _requireGpu(True)
        self.max_batch = int(max_batch)
        self.frame_size = (int(frame_size[0]), int(frame_size[1]))
        self.owner, self.core = _core(model)
        self._parts = encoder_parts(model) if route is None else None
        self._route = ROUTE_BLOCKS if self._parts is not None else ROUTE_MODEL  # of calls within max_batch
        self.last_route = None  # the route the most recent call took
        self.device = next(self.core.parameters()).device
        if self.device.type != "cuda":
            raise C.SrlzError("StateEncoder: the model must live on the GPU (there is no CPU path)")
        if self._parts is None:
            from preprocessing.preprocess import getNChannels
            self.channels = getNChannels()
            return
        stack, head = self._parts
        self._convs, self._bns, self._head = (stack[0], stack[4], stack[8]), (stack[1], stack[5], stack[9]), head
        self.channels = self._convs[0].weight.shape[1]
        self.state_dim = head.weight.shape[0]
        h, w = self.frame_size
        m, c, dev = self.max_batch, self.channels, self.device
        # the tensor the convolution sees is the reference's [N,C,W,H] (preprocessing/data_loader.py:255): rows = image columns
        hi, wi = w, h
        self._in_strides = (h * w * c, 1, c, w * c) if self.frame_layout == "nhwc" else (c * w * h, w * h, h, 1)
        self._dims = []
        cin, kinds = c, (ops.INFER_IN, ops.INFER_MID, ops.INFER_LAST)
        for kind in kinds:
            d = ops.infer_desc(kind, 1, cin, hi, wi, self._in_strides if kind == ops.INFER_IN else None)
            try:
                _, _, hp, wp = ops.infer_out_dims(d)
            except C.SrlzError as e:
                raise ValueError("frames of %d x %d with %d channels do not pass encoder block %d: %s" % (h, w, c, kind, e))
            self._dims.append((cin, hi, wi, hp, wp))
            cin, hi, wi = 64, hp, wp
        k = 64 * self._dims[2][3] * self._dims[2][4]
        if head.weight.shape[1] != k:
            raise ValueError("frames of %d x %d leave %d features, the state head takes %d" % (h, w, k, head.weight.shape[1]))
        self._k = k
        # one descriptor per (block, n): a call builds nothing
        self._descs = [[ops.infer_desc(kind, n, dm[0], dm[1], dm[2], self._in_strides if kind == ops.INFER_IN else None)
                        for kind, dm in zip(kinds, self._dims)] for n in range(1, m + 1)]
        shape = (m, h, w, c) if self.frame_layout == "nhwc" else (m, c, w, h)
        self._frames = torch.empty(shape, dtype=torch.uint8, device=dev)
        self._pin_in = torch.empty(shape, dtype=torch.uint8).pin_memory()
        self._acts = [torch.empty((m, dm[3], dm[4], 64), dtype=torch.float32, device=dev) for dm in self._dims[:2]]
        self._acts.append(torch.empty((m, k), dtype=torch.float32, device=dev))
        self._states = torch.empty((m, self.state_dim), dtype=torch.float32, device=dev)
        self._pin_out = torch.empty((m, self.state_dim), dtype=torch.float32).pin_memory()
        self._wpacks = [torch.empty(C.infer_packed_floats(kind, dm[0]), dtype=torch.float32, device=dev) for kind, dm in zip(kinds, self._dims)]
        self._bnps = [torch.empty(256, dtype=torch.float32, device=dev) for _ in range(3)]
        self._ws_bytes = [C.linear_workspace(n, self.state_dim, k) for n in range(1, m + 1)]
        self._ws = torch.empty(max(max(self._ws_bytes), 16), dtype=torch.uint8, device=dev)
        self._lut = ops.norm_lut(dev)
        self.refresh()

    @classmethod
    def from_log_folder(cls, log_folder, max_batch=32, frame_layout="nhwc", frame_size=(224, 224), valid_models=None):
        """The encoder of a trained experiment: <log_folder>/exp_config.json + srl_model.pth (SRL4robotics.loadSavedModel)."""
        check_layout(frame_layout)
        from models.learner import SRL4robotics, _requireGpu
        _requireGpu(True)
        if valid_models is None:
            valid_models = ["forward", "inverse", "reward", "priors", "episode-prior", "reward-prior", "triplet", "autoencoder", "vae",
                            "perceptual", "dae", "random"]
        if not log_folder.endswith("/"):
            log_folder += "/"
        srl, _ = SRL4robotics.loadSavedModel(log_folder, valid_models, cuda=True)
        srl.model.eval()
        return cls(srl.model, max_batch=max_batch, frame_layout=frame_layout, frame_size=frame_size)

    @property
    def route(self):
        """The route of the most recent call ("model" after a call of more than max_batch frames); before any call, the route that
        calls within max_batch take."""
        return self.last_route or self._route

    def refresh(self):
        """Re-read the convolution weights, the BatchNorm parameters and running statistics and the head (after more training, or a
        load_state_dict): three packing launches and three record launches into the buffers made at construction."""
        if self._route != ROUTE_BLOCKS:
            return
        kinds = (ops.INFER_IN, ops.INFER_MID, ops.INFER_LAST)
        for kind, conv, bn, wpack, bnp in zip(kinds, self._convs, self._bns, self._wpacks, self._bnps):
            ops.infer_pack(conv.weight, kind, out=wpack)
            g, b, rm, rv = [ops._check(t.detach(), "BatchNorm parameter") for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)]
            C.bn_eval_params(C.ptr(g), C.ptr(b), C.ptr(rm), C.ptr(rv), float(bn.eps), C.ptr(bnp), C.stream())
        self._head_w = ops._check(self._head.weight.detach(), "state head weight")
        self._head_b = ops._check(self._head.bias.detach(), "state head bias") if self._head.bias is not None else None

    # ---------------------------------------------------------------------------------------------------------
    def _device_frames(self, frames, n, batched):
        """The call's frames as a contiguous uint8 device tensor [n, ...]: the caller's own when it already is one, else a copy into
        the encoder's staging buffer (host frames travel through the pinned one)."""
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if not batched:
            frames = frames.unsqueeze(0)
        if frames.device.type == "cuda":
            if frames.is_contiguous():
                return frames
            self._frames[:n].copy_(frames)
            return self._frames[:n]
        self._pin_in[:n].copy_(frames)
        self._frames[:n].copy_(self._pin_in[:n], non_blocking=True)
        return self._frames[:n]

    def _model_states(self, frames, single):
        """Route "model": getStates of the model itself, eval mode, no graph, every module's mode put back."""
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if single:
            frames = frames.unsqueeze(0)
        frames = frames.to(self.device)
        x = ops.normalize_u8(frames) if self.frame_layout == "nhwc" else ops.frames_as_float(frames.contiguous())
        modes = [(m, m.training) for m in self.owner.modules()]
        self.owner.eval()
        try:
            with torch.no_grad():
                states = self.owner.getStates(x)
        finally:
            for m, was in modes:
                m.training = was
        return states[0] if single else states

    def __call__(self, frames):
        n, single = check_frames(frames, self.frame_layout, self.channels, self.frame_size)
        if self._route != ROUTE_BLOCKS or n > self.max_batch:
            self.last_route = ROUTE_MODEL
            return self._model_states(frames, single)
        self.last_route = ROUTE_BLOCKS
        x = self._device_frames(frames, n, not single)
        d = self._descs[n - 1]
        ops.infer_block(x, self._wpacks[0], self._bnps[0], self._acts[0], d[0], lut=self._lut)
        ops.infer_block(self._acts[0], self._wpacks[1], self._bnps[1], self._acts[1], d[1])
        ops.infer_block(self._acts[1], self._wpacks[2], self._bnps[2], self._acts[2], d[2])
        C.linear_fwd(C.ptr(self._acts[2]), C.ptr(self._head_w), C.ptr(self._head_b), C.ptr(self._states), n, self.state_dim, self._k, 0,
                     C.ptr(self._ws), self._ws_bytes[n - 1], C.stream())
        return self._states[0] if single else self._states[:n]

    def numpy(self, frames):
        """The states on the host: one copy through the pinned buffer, one synchronisation of the current stream."""
        states = self(frames)
        if self.last_route != ROUTE_BLOCKS:
            return states.detach().cpu().numpy()
        out = self._pin_out[0] if states.dim() == 1 else self._pin_out[:states.shape[0]]
        out.copy_(states, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return out.numpy().copy()


# =============================================================================================================
# Deployment decoder: states to camera frames in six launches.
#
#     dec = FrameDecoder(model, max_batch=32, frame_layout="nhwc", bgr=False)   # SRLModules / SRLModulesSplit / a bare CNNAutoEncoder, CNNVAE
#     dec = FrameDecoder.from_log_folder("logs/<dataset>/<experiment>/")
#     frames  = dec(states)          # [N,S] or [S], numpy or device tensor -> uint8 [N,H,W,C] / [H,W,C]  ("planar": [N,C,W,H] / [C,W,H])
#     decoded = dec.decoded(states)  # fp32 [N,C,W,H]: what model.decode returns in eval mode
#     frames  = dec.numpy(states)    # the bytes on the host through a pinned buffer, one synchronisation
#     dec.refresh(); dec.route       # as StateEncoder
#     reconstruct(encoder, decoder, frames)   # decoder(encoder(frames)), the states never leave the device
#
# States to pictures is srl_model.decode(state) + deNormalize (evaluation/enjoy_latent.py:21-39), which ran the training route in eval
# mode: the linear layer, five ConvTranspose launches on tiles sized for 512 images, four eval BatchNorm records and their
# applications inside autograd Functions, and a picture kernel on top.  Route "blocks" is decoder_fc on srlz_linear_fwd, then each
# decoder block (ConvTranspose 3x3 s2, bias, eval BatchNorm, ReLU: models/models.py:65-83) as ONE launch of csrc/infer_dec.hip, then the
# 4x4 layer, whose epilogue writes either the decode tensor or the picture's bytes in the stated layout.  It computes core.decode(states),
# what enjoy_latent.getImage calls: no split mask.
#
# Route "model" is the model's own decode under no_grad in eval mode, every module's mode restored, and the bytes made from its tensor
# by the same expression (bytes_from_decoded): the dense auto-encoders (their flat output viewed [N,C,W,H], chosen by class) and calls
# of more than max_batch states.  A model without a decoder raises ValueError.
#
# A "blocks" call allocates no device memory, builds no autograd graph, touches neither running statistics, num_batches_tracked, module
# modes nor torch's RNG, and runs on the current stream.  What it returns is a view of the decoder's own buffer, valid until the next call.
# =============================================================================================================
def decoder_parts(model):
    """(decoder_fc's Linear, decoder_conv) of a model whose decode is Linear + conv decoder; None for the dense auto-encoders (route
    "model": they own a conv stack they never run, so this goes by class); ValueError for a model without a decoder."""
    from models.autoencoders import CNNAutoEncoder, LinearAutoEncoder, DenseAutoEncoder
    from models.vae import CNNVAE, DenseVAE
    _, core = _core(model)
    if isinstance(core, (CNNAutoEncoder, CNNVAE)):
        return core.decoder_fc[0], core.decoder_conv
    if isinstance(core, (LinearAutoEncoder, DenseAutoEncoder, DenseVAE)):
        return None
    raise ValueError("%s has no decoder: a FrameDecoder needs an auto-encoder or a VAE" % type(core).__name__)


def decode_route_for(model):
    """The route a FrameDecoder of `model` takes for calls within max_batch (host only); ValueError without a decoder."""
    return ROUTE_BLOCKS if decoder_parts(model) is not None else ROUTE_MODEL


def check_states(states, state_dim):
    """Validate a call's states: floating point, [N,S] or [S] with S = state_dim, at least one.  Returns (n, single)."""
    if not isinstance(states, (np.ndarray, torch.Tensor)):
        raise ValueError("states must be a numpy array or a torch tensor, got %s" % type(states).__name__)
    is_float = np.issubdtype(states.dtype, np.floating) if isinstance(states, np.ndarray) else states.dtype.is_floating_point
    if not is_float:
        raise ValueError("states must be floating point (got %s)" % (states.dtype,))
    shape = tuple(states.shape)
    if len(shape) not in (1, 2):
        raise ValueError("states must be [N,S] or [S], got shape %s" % (shape,))
    single = len(shape) == 1
    n, s = (1, shape[0]) if single else shape
    if s != state_dim:
        raise ValueError("states of shape %s are %d wide, the decoder takes state_dim = %d" % (shape, s, state_dim))
    if n < 1:
        raise ValueError("no state in the call")
    return n, single


_MEAN, _STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def bytes_from_decoded(decoded, frame_layout, bgr=False):
    """The bytes of route "model": the expression of srlz_infer_dec_out on a decode tensor fp32 [N,C,W,H] — x * std, + mean (two fp32
    roundings), clip, rint(x * 255), NaN -> 0 — as uint8 [N,H,W,C] ("nhwc") or [N,C,W,H] ("planar")."""
    check_layout(frame_layout)
    c = decoded.shape[1]
    std = torch.tensor([_STD[i % 3] for i in range(c)], dtype=torch.float32, device=decoded.device).view(1, c, 1, 1)
    mean = torch.tensor([_MEAN[i % 3] for i in range(c)], dtype=torch.float32, device=decoded.device).view(1, c, 1, 1)
    v = torch.clamp(decoded * std + mean, 0.0, 1.0)
    b = torch.nan_to_num(torch.round(v * 255.0), nan=0.0).to(torch.uint8)
    if bgr:
        b = b[:, [3 * (i // 3) + 2 - i % 3 for i in range(c)]]
    return b.permute(0, 3, 2, 1).contiguous() if frame_layout == "nhwc" else b.contiguous()


class FrameDecoder(object):
    MAP = 6  # decoder_fc writes [N, 64, 6, 6] (autoencoders.py:111-118)

    def __init__(self, model, max_batch=32, frame_layout="nhwc", bgr=False, route=None):
        """model: SRLModules / SRLModulesSplit / a bare CNNAutoEncoder, CNNVAE (the dense auto-encoders: route "model").
        bgr: the three channels of each camera reversed (what cv2 shows).  route="model" forces the fallback for every call
        (tools/kb_decode.py measures the two routes side by side); None picks by model class."""
        self.frame_layout = check_layout(frame_layout)
        if route not in (None, ROUTE_MODEL):
            raise ValueError("route must be None or 'model', got %r" % (route,))
        if int(max_batch) < 1:
            raise ValueError("max_batch must be at least 1, got %r" % (max_batch,))
        parts = decoder_parts(model)  # (ValueError for a model without a decoder, before anything touches a GPU)
        from models.learner import _requireGpu
        _requireGpu(True)
        self.max_batch, self.bgr = int(max_batch), bool(bgr)
        self.owner, self.core = _core(model)
        self._parts = parts if route is None else None
        self._route = ROUTE_BLOCKS if self._parts is not None else ROUTE_MODEL
        self.last_route = None
        self.device = next(self.core.parameters()).device
        if self.device.type != "cuda":
            raise C.SrlzError("FrameDecoder: the model must live on the GPU (there is no CPU path)")
        first = parts[0] if parts is not None else self.core.decoder[0]
        self.state_dim = first.in_features
        if self._parts is None:
            from preprocessing.preprocess import getNChannels
            self.channels = getNChannels()
            return
        fc, stack = self._parts
        self._fc, self._convs, self._bns = fc, tuple(stack[i] for i in (0, 3, 6, 9, 12)), tuple(stack[i] for i in (1, 4, 7, 10))
        if fc.out_features != 64 * self.MAP * self.MAP:
            raise ValueError("decoder_fc writes %d features, the decoder blocks take 64 x %d x %d" % (fc.out_features, self.MAP, self.MAP))
        self.channels = c = self._convs[4].weight.shape[1]
        m, dev, s = self.max_batch, self.device, self.state_dim
        kinds = (ops.INFER_DEC_FIRST, ops.INFER_DEC_MID, ops.INFER_DEC_MID, ops.INFER_DEC_MID, ops.INFER_DEC_OUT)
        self._kinds, self._maps, h = kinds, [], self.MAP
        for kind in kinds:
            try:
                ho, _ = ops.infer_dec_out_dims(ops.infer_dec_desc(kind, 1, h, h, c_out=c if kind == ops.INFER_DEC_OUT else 64))
            except C.SrlzError as e:
                raise ValueError("a decoder of %d channels does not pass layer kind %d: %s" % (c, kind, e))
            self._maps.append((h, ho))
            h = ho
        self.frame_size = (h, h)  # (H, W); the decode tensor is [N,C,W,H]
        # element strides (n, c, y, x) of the decode tensor [N,C,W,H] in the picture: byte (n, Y, X, c) of a camera frame is decoded[n][c][X][Y]
        hh = ww = h
        self._out_strides = (hh * ww * c, 1, c, ww * c) if self.frame_layout == "nhwc" else (c * ww * hh, ww * hh, hh, 1)
        # one descriptor per (layer, n): a call builds nothing
        self._descs = [[ops.infer_dec_desc(kind, n, hi, hi) for kind, (hi, _) in zip(kinds[:4], self._maps[:4])] for n in range(1, m + 1)]
        hi = self._maps[4][0]
        self._desc_f32 = [ops.infer_dec_desc(ops.INFER_DEC_OUT, n, hi, hi, c_out=c) for n in range(1, m + 1)]
        self._desc_u8 = [ops.infer_dec_desc(ops.INFER_DEC_OUT, n, hi, hi, c_out=c, out_u8=True, bgr=self.bgr, out_strides=self._out_strides)
                         for n in range(1, m + 1)]
        self._states = torch.empty((m, s), dtype=torch.float32, device=dev)
        self._pin_in = torch.empty((m, s), dtype=torch.float32).pin_memory()
        self._h0 = torch.empty((m, fc.out_features), dtype=torch.float32, device=dev)
        self._acts = [torch.empty((m, ho, ho, 64), dtype=torch.float32, device=dev) for _, ho in self._maps[:4]]
        self._decoded = torch.empty((m, c, h, h), dtype=torch.float32, device=dev)
        shape = (m, h, h, c) if self.frame_layout == "nhwc" else (m, c, h, h)
        self._frames = torch.empty(shape, dtype=torch.uint8, device=dev)
        self._pin_out = torch.empty(shape, dtype=torch.uint8).pin_memory()
        self._wpacks = [torch.empty(C.infer_dec_packed_floats(kind, cv.weight.shape[1]), dtype=torch.float32, device=dev)
                        for kind, cv in zip(kinds, self._convs)]
        self._biases = [torch.zeros(cv.weight.shape[1], dtype=torch.float32, device=dev) for cv in self._convs]
        self._bnps = [torch.empty(256, dtype=torch.float32, device=dev) for _ in range(4)]
        self._fc_w = torch.empty((fc.out_features, s), dtype=torch.float32, device=dev)
        self._fc_b = torch.zeros(fc.out_features, dtype=torch.float32, device=dev)
        self._ws_bytes = [C.linear_workspace(n, fc.out_features, s) for n in range(1, m + 1)]
        self._ws = torch.empty(max(max(self._ws_bytes), 16), dtype=torch.uint8, device=dev)
        self.refresh()

    @classmethod
    def from_log_folder(cls, log_folder, max_batch=32, frame_layout="nhwc", bgr=False, valid_models=None):
        """The decoder of a trained experiment: <log_folder>/exp_config.json + srl_model.pth (SRL4robotics.loadSavedModel)."""
        check_layout(frame_layout)
        from models.learner import SRL4robotics, _requireGpu
        _requireGpu(True)
        if valid_models is None:
            valid_models = ["forward", "inverse", "reward", "priors", "episode-prior", "reward-prior", "triplet", "autoencoder", "vae",
                            "perceptual", "dae", "random"]
        if not log_folder.endswith("/"):
            log_folder += "/"
        srl, _ = SRL4robotics.loadSavedModel(log_folder, valid_models, cuda=True)
        srl.model.eval()
        return cls(srl.model, max_batch=max_batch, frame_layout=frame_layout, bgr=bgr)

    @property
    def route(self):
        """The route of the most recent call ("model" after a call of more than max_batch states); before any call, the route that
        calls within max_batch take."""
        return self.last_route or self._route

    def refresh(self):
        """Re-read decoder_fc, the ConvTranspose weights and biases, the BatchNorm parameters and running statistics (after more
        training, or a load_state_dict) into the buffers made at construction: five packing launches, four record launches, copies."""
        if self._route != ROUTE_BLOCKS:
            return
        with torch.no_grad():
            self._fc_w.copy_(self._fc.weight.detach())
            if self._fc.bias is not None:
                self._fc_b.copy_(self._fc.bias.detach())
            for kind, conv, wpack, bias in zip(self._kinds, self._convs, self._wpacks, self._biases):
                ops.infer_dec_pack(conv.weight, kind, out=wpack)
                if conv.bias is not None:
                    bias.copy_(conv.bias.detach())
        for bn, bnp in zip(self._bns, self._bnps):
            g, b, rm, rv = [ops._check(t.detach(), "BatchNorm parameter") for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)]
            C.bn_eval_params(C.ptr(g), C.ptr(b), C.ptr(rm), C.ptr(rv), float(bn.eps), C.ptr(bnp), C.stream())

    # ---------------------------------------------------------------------------------------------------------
    def _device_states(self, states, n, single):
        """The call's states as a contiguous fp32 device tensor [n, S]: the caller's own when it already is one, else a copy into the
        decoder's staging buffer (host states travel through the pinned one)."""
        if isinstance(states, np.ndarray):
            states = torch.from_numpy(np.ascontiguousarray(states))
        if single:
            states = states.unsqueeze(0)
        if states.device.type == "cuda":
            if states.is_contiguous() and states.dtype == torch.float32:
                return states.detach()
            self._states[:n].copy_(states.detach())
            return self._states[:n]
        self._pin_in[:n].copy_(states.detach())
        self._states[:n].copy_(self._pin_in[:n], non_blocking=True)
        return self._states[:n]

    def _model_decoded(self, states, single):
        """Route "model": decode of the model itself, eval mode, no graph, every module's mode put back -> fp32 [n,C,W,H]."""
        if isinstance(states, np.ndarray):
            states = torch.from_numpy(np.ascontiguousarray(states))
        if single:
            states = states.unsqueeze(0)
        states = states.detach().to(self.device, torch.float32).contiguous()
        modes = [(m, m.training) for m in self.owner.modules()]
        self.owner.eval()
        try:
            with torch.no_grad():
                dec = self.core.decode(states)
        finally:
            for m, was in modes:
                m.training = was
        if dec.dim() == 2:  # the dense auto-encoders decode into the flat vector BaseModelAutoEncoder.forward views as the input's shape
            from preprocessing.preprocess import IMAGE_WIDTH, IMAGE_HEIGHT
            dec = dec.view(dec.size(0), self.channels, IMAGE_WIDTH, IMAGE_HEIGHT)
        return dec

    def _blocks(self, states, n, single):
        """Five of the six launches: decoder_fc and the four blocks; the last block's activations are self._acts[3][:n]."""
        x = self._device_states(states, n, single)
        C.linear_fwd(C.ptr(x), C.ptr(self._fc_w), C.ptr(self._fc_b), C.ptr(self._h0), n, self._h0.shape[1], self.state_dim, 0,
                     C.ptr(self._ws), self._ws_bytes[n - 1], C.stream())
        d, src = self._descs[n - 1], self._h0
        for i in range(4):
            ops.infer_dec_block(src, self._wpacks[i], self._biases[i], self._bnps[i], self._acts[i], d[i])
            src = self._acts[i]
        return src

    def _takes_blocks(self, n):
        self.last_route = ROUTE_BLOCKS if self._route == ROUTE_BLOCKS and n <= self.max_batch else ROUTE_MODEL
        return self.last_route == ROUTE_BLOCKS

    def decoded(self, states):
        """fp32 [N,C,W,H] ([C,W,H] for one bare state): what model.decode returns in eval mode."""
        n, single = check_states(states, self.state_dim)
        if not self._takes_blocks(n):
            dec = self._model_decoded(states, single)
        else:
            ops.infer_dec_out(self._blocks(states, n, single), self._wpacks[4], self._biases[4], self._decoded, self._desc_f32[n - 1])
            dec = self._decoded[:n]
        return dec[0] if single else dec

    def __call__(self, states):
        """uint8 [N,H,W,C] ("nhwc") or [N,C,W,H] ("planar"); one bare state gives one bare frame."""
        n, single = check_states(states, self.state_dim)
        if not self._takes_blocks(n):
            frames = bytes_from_decoded(self._model_decoded(states, single), self.frame_layout, self.bgr)
        else:
            ops.infer_dec_out(self._blocks(states, n, single), self._wpacks[4], self._biases[4], self._frames, self._desc_u8[n - 1])
            frames = self._frames[:n]
        return frames[0] if single else frames

    def numpy(self, states):
        """The frames on the host: one copy through the pinned buffer, one synchronisation of the current stream."""
        frames = self(states)
        if self.last_route != ROUTE_BLOCKS:
            return frames.cpu().numpy()
        out = self._pin_out[0] if frames.dim() == 3 else self._pin_out[:frames.shape[0]]
        out.copy_(frames, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return out.numpy().copy()


def reconstruct(encoder, decoder, frames):
    """decoder(encoder(frames)): camera frames through the state and back with no host round trip — the decoder reads the encoder's
    state buffer in place.  Bit-identical to the two calls made separately."""
    return decoder(encoder(frames))
