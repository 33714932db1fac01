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
of this file; LatentDynamics — states and plans through the forward and reward heads to returns in one launch — imagine, and the
planner LatentDynamics.plan — a cross-entropy search on the device, one launch per iteration — are the third part.
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


# =============================================================================================================
# Deployment dynamics: states and plans to final states and returns in one launch.
#
#     dyn = LatentDynamics(model, max_rows=8192, max_horizon=32)   # SRLModules / SRLModulesSplit / a learner
#     dyn = LatentDynamics.from_log_folder("logs/<dataset>/<experiment>/")
#     dyn.heads                      # subset of ("forward", "inverse", "reward") the model's losses trained
#     dyn.route                      # "rollout" or "model", as StateEncoder.route
#     nxt = dyn.step(states, actions)              # [N,S], [N] -> [N,S]: the same kernel with K = T = 1
#     out = dyn.rollout(states, plans, gamma=1.0, keep_trajectory=False, keep_logits=False)
#     out.final_states, out.returns, out.trajectory, out.reward_logits, out.best   # [N,K,S], [N,K], [N,K,T,S], [N,K,T,2], [N]
#     a = dyn.act(states, plans)                   # first action of each environment's best plan, [N] int64, no host synchronisation
#     dyn.reward_logits(states, next_states); dyn.action_logits(states, next_states)   # the model's own heads under no_grad
#     frames = imagine(dyn, decoder, states, plans)   # the trajectories through a FrameDecoder
#
# What sits between StateEncoder and FrameDecoder: the three heads every srl_model.pth carries (models/forward_inverse.py).  A
# controller on the learned state scores K candidate action sequences per environment by rolling each through forwardModel and asking
# rewardModel at every step.  A rollout IS that composition of the owner's own methods under no_grad:
#     s' = owner.forwardModel(s, a_t);  l_t = owner.rewardModel(s, s');  ret += g * softmax(l_t)[1];  g *= gamma;  s = s'
# which through the training kernels is six launches and six temporaries a step.  Route "rollout" runs all N * K rows and all T steps
# as ONE launch of csrc/rollout.hip, the state tile on chip throughout, the weights read in place from the model's own parameters (no
# refresh(): further training is seen by the next call).  It serves SRLModules of every model_type — the heads do not depend on the
# encoder.  Route "model" computes the composition above step by step: SRLModulesSplit (whose heads see masked states), head shapes
# srlz_rollout_supported refuses, and calls of more than max_rows rows or max_horizon steps.  Nothing is rejected for size, nothing is
# approximated.
#
# plans: integers [N,K,T], or [K,T] shared by every environment (read with a stride of 0, never tiled), or one bare [T]; states [N,S] or
# one bare [S]; numpy or device tensors.  Outputs drop the axes the inputs did not have.  Host plans are range-checked here; on the
# device an action outside [0, A) turns its row NaN from that step on (include/srlz.h).  returns, reward_logits and best need the
# reward head and are None without it; best = argmax_k returns, ties to the lowest k, NaN returns never chosen over a number.
# Using a head the model's losses did not train raises ValueError; untrained_ok=True overrides it.  A module without .losses allows all.
#
# A "rollout" call launches on the current stream into buffers made at construction (states, plans, final states, returns, and the
# trajectory / logits buffers of max_rows * max_horizon steps), builds no graph, and leaves modes, parameters and torch's RNG alone.
# What it returns are views of those buffers, valid until the next call.
#
# The planner.  act scores plans the caller brings; a controller has a state and wants an action:
#     p = dyn.plan(states, horizon, n_plans=64, iterations=4, elites=8, sharpness=8, gamma=1.0, seed=0, init_weights=None,
#                  keep_population=False)
#     p.best_plan, p.best_return, p.action, p.weights     # int32 [N,T], fp32 [N], int64 [N] (= best_plan[:, 0]), int32 [N,T,A]
#     p.plans, p.returns                                  # keep_population: int32 [I,N,K,T], fp32 [I,N,K]; else None
#     p.shifted()                                         # the table one step ahead: the next call's init_weights
# A categorical cross-entropy method over discrete action sequences, stated exactly in include/srlz.h: a table of integer weights
# per (environment, step, action), uniform or the caller's init_weights ([T,A] or [N,T,A]); each of `iterations` rounds samples
# n_plans plans per environment from it (Philox4x32-10, counter (t >> 2, k, n, i), key = the 64-bit seed), rolls them as rollout
# does, ranks them (return descending — NaN as -inf — then k ascending), keeps the best plan seen so far (replaced only by a strictly
# greater key) and refits the table to w = 1 + sharpness * (elites with that action at that step).  Everything but the returns is
# integer arithmetic: a call is a function of its inputs and the seed, bit for bit.  Route "rollout" is `iterations` launches of
# csrc/plan.hip back to back on the current stream, no host synchronisation between them and no plan on the host; the returns are the
# bits dyn.rollout gives for the same plans.  Route "model" runs the same algorithm in numpy (cem_host) over this object's own
# returns (_run): SRLModulesSplit, shapes srlz_plan_supported refuses (more than 256 actions, 1024 plans or 32 steps) and calls of
# more than max_rows rows — nothing is rejected for size.  The reward head is required (the gating ValueError of act).  The planner's
# buffers are made on the first plan call and grown only when a call asks for more; what a call returns are views of them, valid
# until the next call (shifted() is a new tensor).  Device init_weights — a Plan's shifted() — are taken as they are; host ones are
# checked: non-negative, every row with a positive total.
#
# Goals.  "Drive the learned state to the state of this goal picture":
#     out = dyn.rollout(states, plans, gamma=1.0, goal=g, goal_weight=1.0, goal_mode="running", keep_goal_dist=False)
#     out.returns, out.best, out.goal_dist            # the score [N,K], its argmax [N], |s_{t+1} - goal|^2 [N,K,T]
#     a = dyn.act(states, plans, goal=g, goal_mode="final")
#     p = dyn.plan(states, horizon, ..., goal=g, goal_weight=1.0, goal_mode="running")   # p.best_return, p.returns are scores
#     p = reach(encoder, dyn, frames, goal_frames, horizon, **plan_kwargs)               # from camera frames, on the device
# goal: floating point [S] (shared, read with a stride of 0) or [N,S], numpy or a device tensor.  Per step (include/srlz.h):
#     d_t = |s_{t+1} - goal|^2;  c_t = d_t ("running") | d_t at the last step alone ("final");  term_t = prob_t - w c_t, or -w c_t
#     without a reward head;  score = sum_t g_t term_t
# With a goal only the forward head is required: a reward head the losses trained joins the score, an untrained one only under
# untrained_ok.  Route "rollout" is srlz_rollout_goal / srlz_plan_cem_goal — the same tile with its goal term compiled in, the same
# bits for the states and logits — where goal_route_for / plan_goal_route_for say so and within max_rows / max_horizon; otherwise
# route "model": the model's own forwardModel / rewardModel step by step, scored by goal_scores (the rule written once, numpy or
# torch), which also feeds cem_host.  A call without a goal takes exactly the path it always took.
#
# Tree search.  The actions of this zoo are discrete and few; where the tree fits, search it instead of sampling it:
#     r = dyn.search(states, horizon, beam=64, gamma=1.0, keep_leaves=False, goal=None, goal_weight=1.0, goal_mode="running")
#     r.best_plan, r.best_return, r.action      # int32 [N,T], fp32 [N], int64 [N] (= best_plan[:, 0]); no host synchronisation
#     r.exact, r.expanded, r.leaves             # nothing was pruned; forward steps per environment (sum of C_t); L
#     r.leaf_plans, r.leaf_returns              # keep_leaves: int32 [N,L,T], fp32 [N,L]; else None
#     p = reach(encoder, dyn, frames, goal_frames, horizon, planner="search", beam=64)
# Level by level (include/srlz.h states it exactly): every node of the frontier is expanded by every action, child c = f * A + a;
# while the children are at most `beam` all of them go on, otherwise the `beam` best by (ret descending — NaN as -inf — then c
# ascending); the leaves are the last level's children, best the greatest among them, ties to the lowest c.  A prefix is expanded
# once: A + A^2 + .. + A^T forward steps for all A^T leaves where rollout over the enumerated plans runs T * A^T.  With
# beam >= A^(T-1) nothing is pruned (exact): the leaves are all A^T plans in lexicographic order and best_plan is the optimum under
# the model — what plan() approaches by sampling.  Route "rollout" is `horizon` launches of csrc/beam.hip back to back on the current
# stream; every leaf's return has the bits dyn.rollout gives for that leaf's plan (with the same goal, weight and mode).  Where
# search_route_for says so — SRLModulesSplit, shapes srlz_beam_supported refuses (beam * A beyond 8192, more than 32 steps) and calls
# of more than max_rows children a level — route "model" runs the same algorithm in numpy (beam_host) over this object's own returns
# of the prefix plans (_run / _run_goal).  Heads and goals are gated as in plan; buffers are made on the first search call and grown
# on demand; what a call returns are views of them, valid until the next call.
#
# The dynamics' own metric.  Whether a trained forward head still means anything after `horizon` steps — the open-loop check on a
# recorded sequence, which plan(horizon=...) rests on:
#     h = dyn.horizon_error(states, actions, episode_starts, horizon=10, rewards=None, starts=None, keep_rows=False)
#     h.count, h.mse, h.baseline_mse, h.ratio            # per horizon [T]; ratio below 1: the model beats "nothing moves"
#     h.reward_accuracy, h.majority_accuracy             # with rewards and a trained reward head, else None
#     h.err, h.base, h.logits                            # keep_rows: the rows [M,T], [M,T], [M,T,2]
# From every start frame i the recorded actions a_i .. a_{i+L-1} go through the forward head, L = valid_steps: as far as the episode
# and the horizon reach; the imagined state after t + 1 steps is compared with the recorded states[i + t + 1], next to the error of
# "the state stays states[i]"; the reward head, on the imagined pairs, is asked for the reward stored at each transition's first
# frame (-1 read as 0, the learner's own labelling).  mse = sum_err / (count * S), ratio = sum_err / sum_base.  Route "rollout" is
# two launches of csrc/horizon.hip (include/srlz.h states every sum's order): the imagined states never leave the chip, and max_rows
# does not apply — nothing is staged per row.  Route "model" is the model's own forwardModel / rewardModel step by step with fp64
# sums on the host: SRLModulesSplit, head shapes srlz_horizon_supported refuses, horizons beyond 32 or max_horizon.
#
# A forward head without training.  The head is one Linear under an MSE: over a recording its minimiser is a linear solve
# (srlz/dynfit.py, csrc/dynfit.hip), so any representation with recorded actions can be rolled, planned and measured:
#     dyn = LatentDynamics.from_recording(states, actions, episode_starts, n_actions=None, ridge=1e-6, starts=None)
#     fit = dyn.refit_forward(states, actions, episode_starts, ridge=1e-6, starts=None)     # a model's own head, in place
#     fit.weight, fit.bias, fit.weight64, fit.bias64, fit.count, fit.gram, fit.cross, fit.route
#
# A reward head without training.  The reward head is a three-layer classifier: its optimum has no closed form, so it is trained on
# the recording with Adam, one launch per epoch (srlz/headfit.py, csrc/headfit.hip).  With it a recording's dynamics
# roll, plan and search by reward, without a goal:
#     dyn = LatentDynamics.from_recording(states, actions, episode_starts, rewards=rewards, reward_fit=dict(epochs=30))
#     rfit = dyn.refit_reward(states, rewards, episode_starts, epochs=30, batch_size=32, lr=0.005, seed=0)   # a model's own head, in place
#     rfit.state_dict, rfit.history, rfit.best_epoch, rfit.count, rfit.val_count, rfit.route
#
# An inverse head without training.  "Can the action be read off (state, next state)?" — this zoo's default loss — has no closed
# form either: Linear(2S, A) under a cross-entropy, trained on the recording with Adam, one launch per epoch (srlz/invfit.py,
# csrc/invfit.hip).  With it action_logits works, and action_accuracy says which actions the representation keeps:
#     dyn = LatentDynamics.from_recording(states, actions, episode_starts, inverse_fit=dict(epochs=30))
#     ifit = dyn.refit_inverse(states, actions, episode_starts, epochs=30, batch_size=32, lr=0.005, seed=0)  # a model's own head, in place
#     ifit.state_dict, ifit.history, ifit.best_epoch, ifit.count, ifit.val_count, ifit.route
#     acc = dyn.action_accuracy(states, actions, episode_starts, starts=None)     # one srlz_invfit_eval launch for a linear head
#     acc.accuracy, acc.majority_accuracy, acc.recall, acc.support, acc.hits, acc.loss, acc.count, acc.route
# =============================================================================================================
ROUTE_ROLLOUT = "rollout"
HEADS = ("forward", "inverse", "reward")


class Rollout(object):
    """What LatentDynamics.rollout returns; a field the call did not ask for (or has no head for) is None."""
    __slots__ = ("final_states", "returns", "trajectory", "reward_logits", "best", "goal_dist")

    def __init__(self, final_states, returns=None, trajectory=None, reward_logits=None, best=None, goal_dist=None):
        self.final_states, self.returns, self.trajectory, self.reward_logits, self.best = final_states, returns, trajectory, reward_logits, best
        self.goal_dist = goal_dist


class ActionAccuracy(object):
    """What LatentDynamics.action_accuracy returns, from the counters of srlz_invfit_eval (rows, correct, bad, support[A], hits[A])."""
    __slots__ = ("count", "accuracy", "majority_accuracy", "recall", "support", "hits", "loss", "route")

    def __init__(self, counts, loss_sum, n_actions, route):
        c = [int(v) for v in counts]
        a = int(n_actions)
        self.count, self.support, self.hits, self.route = c[0], c[3:3 + a], c[3 + a:3 + 2 * a], route
        self.accuracy, self.majority_accuracy = float(c[1]) / c[0], float(max(self.support)) / c[0]
        self.recall = [(float(h) / s if s else None) for h, s in zip(self.hits, self.support)]
        self.loss = loss_sum / c[0]


def _dynamics_owner(model):
    """The module that owns forward_net / inverse_net / reward_net (a learner's .model, or the module itself)."""
    owner, _ = _core(model)
    if getattr(owner, "forward_net", None) is None:
        raise ValueError("%s carries no forward / inverse / reward heads: LatentDynamics needs SRLModules or SRLModulesSplit"
                         % type(owner).__name__)
    return owner


def trained_heads(model):
    """The subset of ("forward", "inverse", "reward") the model's losses trained; all three for a module without .losses."""
    owner = _dynamics_owner(model)
    losses = getattr(owner, "losses", None)
    return HEADS if losses is None else tuple(h for h in HEADS if h in losses)


def check_head(model, head, untrained_ok=False):
    """ValueError when `head` was not trained by the model's losses (unless untrained_ok)."""
    if untrained_ok or head in trained_heads(model):
        return
    raise ValueError("the %s head of this model was never trained: its losses are %s (untrained_ok=True uses the head as it is)"
                     % (head, list(getattr(_dynamics_owner(model), "losses", []))))


def dynamics_dims(model):
    """(S, A, H, n_rewards) of the model's heads; H = n_rewards = 0 when reward_net is not the reference's three-layer head."""
    owner = _dynamics_owner(model)
    fw = owner.forward_net
    s, a = fw.out_features, fw.in_features - fw.out_features
    rn = owner.reward_net
    three = isinstance(rn, torch.nn.Sequential) and len(rn) == 5 and all(isinstance(rn[i], torch.nn.Linear) for i in (0, 2, 4))
    if not three or rn[0].in_features != 2 * s or rn[2].in_features != rn[0].out_features or rn[2].out_features != rn[0].out_features \
            or rn[4].in_features != rn[0].out_features or any(rn[i].bias is None for i in (0, 2, 4)) or fw.bias is None:
        return s, a, 0, 0
    return s, a, rn[0].out_features, rn[4].out_features


def dynamics_route_for(model):
    """The route a LatentDynamics of `model` takes for calls within max_rows and max_horizon (host only: no GPU is asked for)."""
    from models.modules import SRLModules
    owner = _dynamics_owner(model)
    s, a, h, nr = dynamics_dims(model)
    return ROUTE_ROLLOUT if isinstance(owner, SRLModules) and a >= 1 and ops.rollout_supported(s, a, h, nr) else ROUTE_MODEL


def check_plans(plans, n, n_actions):
    """Validate a call's plans: integers, [N,K,T] with N = n, or [K,T], or one bare [T]; host plans within [0, n_actions).
    Returns (k, t, shared, bare): plans per environment, steps, whether one [K,T] serves every environment, whether one bare plan came."""
    if not isinstance(plans, (np.ndarray, torch.Tensor)):
        raise ValueError("plans must be a numpy array or a torch tensor, got %s" % type(plans).__name__)
    is_int = np.issubdtype(plans.dtype, np.integer) if isinstance(plans, np.ndarray) else \
        plans.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)
    if not is_int:
        raise ValueError("plans must be integer actions (got %s)" % (plans.dtype,))
    shape = tuple(plans.shape)
    if len(shape) not in (1, 2, 3):
        raise ValueError("plans must be [N,K,T], [K,T] or [T], got shape %s" % (shape,))
    if len(shape) == 3 and shape[0] != n:
        raise ValueError("plans of shape %s are for %d environments, the call has %d states" % (shape, shape[0], n))
    if min(shape) < 1:
        raise ValueError("plans of shape %s hold no action" % (shape,))
    if isinstance(plans, np.ndarray) or plans.device.type == "cpu":
        lo, hi = int(plans.min()), int(plans.max())
        if lo < 0 or hi >= n_actions:
            raise ValueError("plans must hold actions in [0, %d), got %d .. %d" % (n_actions, lo, hi))
    return (shape[-2] if len(shape) > 1 else 1), shape[-1], len(shape) < 3, len(shape) == 1


# ---- goals: "drive the learned state to the state of this goal picture" (include/srlz.h states the scoring rule) ----
GOAL_MODES = ("running", "final")


def check_goal(goal, n, state_dim):
    """Validate a call's goal: floating point, one [S] shared by every environment or [N,S] with N = n, S = state_dim.
    Returns shared: whether one goal serves every environment."""
    if not isinstance(goal, (np.ndarray, torch.Tensor)):
        raise ValueError("goal must be a numpy array or a torch tensor, got %s" % type(goal).__name__)
    is_float = np.issubdtype(goal.dtype, np.floating) if isinstance(goal, np.ndarray) else goal.dtype.is_floating_point
    if not is_float:
        raise ValueError("goal must be floating point (got %s)" % (goal.dtype,))
    shape = tuple(goal.shape)
    if len(shape) not in (1, 2):
        raise ValueError("goal must be [N,S] or [S], got shape %s" % (shape,))
    if shape[-1] != state_dim:
        raise ValueError("goal of shape %s is %d wide, the dynamics take state_dim = %d" % (shape, shape[-1], state_dim))
    if len(shape) == 2 and shape[0] != n:
        raise ValueError("goal of shape %s is for %d environments, the call has %d states" % (shape, shape[0], n))
    return len(shape) == 1


def check_goal_args(goal_weight, goal_mode):
    """Validate a goal's weight (a finite number > 0) and mode ("running" or "final").  Returns (float weight, mode)."""
    if isinstance(goal_weight, bool) or not isinstance(goal_weight, (int, float, np.integer, np.floating)):
        raise ValueError("goal_weight must be a number, got %r" % (goal_weight,))
    w = float(goal_weight)
    with np.errstate(over="ignore", under="ignore"):
        w32 = float(np.float32(w))  # what the kernel takes
    if not np.isfinite(w32) or not w32 > 0:
        raise ValueError("goal_weight must be finite and > 0 (as a float32), got %r" % (goal_weight,))
    if goal_mode not in GOAL_MODES:
        raise ValueError("goal_mode must be 'running' or 'final', got %r" % (goal_mode,))
    return w, goal_mode


def goal_scores(trajectory, goal, probs=None, gamma=1.0, goal_weight=1.0, goal_mode="running"):
    """The scoring rule of include/srlz.h on a whole trajectory, in the trajectory's own arithmetic (numpy or torch, any float type):
    trajectory [N,K,T,S] (entry t = s_{t+1}), goal [S] or [N,S], probs [N,K,T] = softmax(reward logits)[1] or None (no reward head).
        d_t = |s_{t+1} - goal|^2;  c_t = d_t (running) | d_t at t = T-1 alone (final);  term_t = probs_t - w c_t  |  -w c_t
        score = sum_t g_t term_t,  g_0 = 1, g_{t+1} = g_t * gamma (gamma as the float32 the kernel takes)
    Returns (scores [N,K], goal_dist [N,K,T]).  What route "model" and the host planner score by; the kernels' order of d_t's sum
    differs, their score's order is this one."""
    w, goal_mode = check_goal_args(goal_weight, goal_mode)
    if torch.is_tensor(trajectory):
        g = torch.as_tensor(goal).to(trajectory.device, trajectory.dtype)
        scalar = lambda v: torch.tensor(float(np.float32(v)), dtype=trajectory.dtype, device=trajectory.device)
    else:
        trajectory = np.asarray(trajectory)
        g = np.asarray(goal.detach().cpu().numpy() if torch.is_tensor(goal) else goal).astype(trajectory.dtype)
        scalar = lambda v: trajectory.dtype.type(np.float32(v))
    g = g.reshape((1, 1, 1, -1)) if g.ndim == 1 else g.reshape((g.shape[0], 1, 1, g.shape[1]))
    diff = trajectory - g
    dist = (diff * diff).sum(-1)
    t = dist.shape[-1]
    wv, gam, disc = scalar(w), scalar(gamma), scalar(1.0)
    score = torch.zeros_like(dist[..., 0]) if torch.is_tensor(dist) else np.zeros_like(dist[..., 0])
    for step in range(t):
        term = None
        if goal_mode == "running" or step == t - 1:
            term = -(wv * dist[..., step]) if probs is None else probs[..., step] - wv * dist[..., step]
        elif probs is not None:
            term = probs[..., step]
        if term is not None:  # (final mode without a reward head: the steps before the last add -0)
            score = score + disc * term
        disc = disc * gam
    return score, dist


# ---- the planner's host side: argument checks, the route table and the same algorithm in numpy (route "model") ----
PLAN_MAX_SHARPNESS = 4096


class Plan(object):
    """What LatentDynamics.plan returns.  best_plan int32 [N,T], best_return fp32 [N], action int64 [N] (= best_plan[:, 0], as act
    returns it), weights int32 [N,T,A] (the final table's integer weights), plans int32 [I,N,K,T] and returns fp32 [I,N,K] (the
    whole population) or None; a bare state drops the N axis everywhere.  All on the device."""
    __slots__ = ("best_plan", "best_return", "action", "weights", "plans", "returns")

    def __init__(self, best_plan, best_return, action, weights, plans=None, returns=None):
        self.best_plan, self.best_return, self.action, self.weights, self.plans, self.returns = \
            best_plan, best_return, action, weights, plans, returns

    def shifted(self):
        """The table moved one step ahead — step 0 dropped, a uniform last step: the init_weights of the controller's next call."""
        w = self.weights
        return torch.cat((w[..., 1:, :], torch.ones_like(w[..., :1, :])), dim=-2)


def check_plan_args(horizon, n_plans, iterations, elites, sharpness, seed):
    """Validate a plan call's numbers (host only).  Returns them as ints: (horizon, n_plans, iterations, elites, sharpness, seed)."""
    vals = []
    for name, v in (("horizon", horizon), ("n_plans", n_plans), ("iterations", iterations), ("elites", elites), ("sharpness", sharpness),
                    ("seed", seed)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s must be an integer, got %r" % (name, v))
        vals.append(int(v))
    t, k, it, e, q, seed = vals
    if t < 1 or k < 1 or it < 1:
        raise ValueError("horizon, n_plans and iterations must be at least 1, got %d, %d and %d" % (t, k, it))
    if not 1 <= e <= k:
        raise ValueError("elites must lie in [1, n_plans = %d], got %d" % (k, e))
    if not 0 <= q <= PLAN_MAX_SHARPNESS:
        raise ValueError("sharpness must lie in [0, %d], got %d" % (PLAN_MAX_SHARPNESS, q))
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be a 64-bit unsigned integer, got %d" % seed)
    return t, k, it, e, q, seed


def check_init_weights(init_weights, n, horizon, n_actions):
    """Validate a plan call's init_weights: None, or integers [T,A] / [N,T,A]; host weights non-negative, below 2^31, every (n, t) row
    with a positive total below 2^32 (device weights — a Plan's shifted() — are taken as they are).  Returns (weights, shared)."""
    if init_weights is None:
        return None, True
    if not isinstance(init_weights, (np.ndarray, torch.Tensor)):
        raise ValueError("init_weights must be a numpy array or a torch tensor, got %s" % type(init_weights).__name__)
    is_int = np.issubdtype(init_weights.dtype, np.integer) if isinstance(init_weights, np.ndarray) else \
        init_weights.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)
    if not is_int:
        raise ValueError("init_weights must be integers (got %s)" % (init_weights.dtype,))
    shape = tuple(init_weights.shape)
    if shape not in ((horizon, n_actions), (n, horizon, n_actions)):
        raise ValueError("init_weights must be [T,A] = %s or [N,T,A] = %s, got shape %s"
                         % ((horizon, n_actions), (n, horizon, n_actions), shape))
    if isinstance(init_weights, np.ndarray) or init_weights.device.type == "cpu":
        host = np.asarray(init_weights).astype(np.int64)
        if host.min() < 0 or host.max() >= 2 ** 31:
            raise ValueError("init_weights must be non-negative and below 2^31, got %d .. %d" % (host.min(), host.max()))
        totals = host.sum(axis=-1)
        if totals.min() < 1 or totals.max() >= 2 ** 32:
            raise ValueError("every row of init_weights needs a positive total below 2^32, got totals %d .. %d" % (totals.min(), totals.max()))
        init_weights = host
    return init_weights, len(shape) == 2


def plan_route_for(model, n_plans, horizon, n_envs=1, max_rows=8192):
    """The route LatentDynamics.plan takes for a call of n_envs states (host only: no GPU is asked for)."""
    if dynamics_route_for(model) != ROUTE_ROLLOUT or n_envs * n_plans > max_rows:
        return ROUTE_MODEL
    s, a, h, nr = dynamics_dims(model)
    return ROUTE_ROLLOUT if ops.plan_supported(s, a, h, nr, n_plans, horizon) else ROUTE_MODEL


def goal_route_for(model, has_goal_only=False):
    """The route a LatentDynamics of `model` takes for calls with a goal within max_rows and max_horizon (host only: no GPU is asked
    for).  has_goal_only: the reward head stays out of the score (never trained, or not the reference's three-layer head)."""
    from models.modules import SRLModules
    owner = _dynamics_owner(model)
    s, a, h, nr = dynamics_dims(model)
    ok = isinstance(owner, SRLModules) and a >= 1 and owner.forward_net.bias is not None and \
        ops.rollout_goal_supported(s, a, h, nr, not has_goal_only)
    return ROUTE_ROLLOUT if ok else ROUTE_MODEL


def plan_goal_route_for(model, has_goal_only, n_plans, horizon, n_envs=1, max_rows=8192):
    """The route LatentDynamics.plan takes for a call of n_envs states with a goal (host only: no GPU is asked for)."""
    if goal_route_for(model, has_goal_only) != ROUTE_ROLLOUT or n_envs * n_plans > max_rows:
        return ROUTE_MODEL
    s, a, h, nr = dynamics_dims(model)
    return ROUTE_ROLLOUT if ops.plan_goal_supported(s, a, h, nr, not has_goal_only, n_plans, horizon) else ROUTE_MODEL


# ---- the tree search's host side: sizes, argument checks, the route table and the same algorithm in numpy (route "model") ----
class Search(object):
    """What LatentDynamics.search returns.  best_plan int32 [N,T], best_return fp32 [N], action int64 [N] (= best_plan[:, 0]);
    exact: nothing was pruned (best_plan is the optimum under the model), expanded: forward steps per environment (the sum of C_t),
    leaves: L; leaf_plans int32 [N,L,T] and leaf_returns fp32 [N,L] (keep_leaves) or None; a bare state drops the N axis everywhere.
    All tensors on the device."""
    __slots__ = ("best_plan", "best_return", "action", "exact", "expanded", "leaves", "leaf_plans", "leaf_returns")

    def __init__(self, best_plan, best_return, action, exact, expanded, leaves, leaf_plans=None, leaf_returns=None):
        self.best_plan, self.best_return, self.action, self.exact, self.expanded, self.leaves, self.leaf_plans, self.leaf_returns = \
            best_plan, best_return, action, exact, expanded, leaves, leaf_plans, leaf_returns


def check_search_args(horizon, beam):
    """Validate a search call's numbers (host only).  Returns them as ints: (horizon, beam)."""
    vals = []
    for name, v in (("horizon", horizon), ("beam", beam)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s must be an integer, got %r" % (name, v))
        vals.append(int(v))
    if vals[0] < 1 or vals[1] < 1:
        raise ValueError("horizon and beam must be at least 1, got %d and %d" % tuple(vals))
    return tuple(vals)


def search_sizes(beam, horizon, n_actions):
    """The tree of a search call, per environment (host only): dict of frontier [T] = F_t, children [T] = C_t = F_t * A (F_0 = 1,
    F_{t+1} = min(C_t, beam)), leaves = L = C_{T-1}, exact (no level before the last has more than `beam` children: beam >= A^(T-1)),
    expanded (forward steps: the sum of C_t)."""
    t, w = check_search_args(horizon, beam)
    a = int(n_actions)
    if a < 1:
        raise ValueError("n_actions must be at least 1, got %d" % a)
    frontier, children, f = [], [], 1
    for _ in range(t):
        frontier.append(f)
        children.append(f * a)
        f = min(f * a, w)
    return dict(frontier=frontier, children=children, leaves=children[-1], exact=all(c <= w for c in children[:-1]),
                expanded=sum(children))


def search_route_for(model, beam, horizon, n_envs=1, max_rows=8192, has_goal_only=False):
    """The route LatentDynamics.search takes for a call of n_envs states (host only: no GPU is asked for).  has_goal_only: the
    reward head stays out of the score, as in goal_route_for.  A beam wider than the tree's widest frontier counts as that frontier."""
    if goal_route_for(model, has_goal_only) != ROUTE_ROLLOUT:
        return ROUTE_MODEL
    s, a, h, nr = dynamics_dims(model)
    t, w = check_search_args(horizon, beam)
    if t > 64:  # (far beyond the kernel's 32 steps; the tree's sizes are not needed to say so)
        return ROUTE_MODEL
    sizes = search_sizes(w, t, a)
    w = max(sizes["frontier"])
    if w * a > 2 ** 20 or n_envs * sizes["leaves"] > max_rows:
        return ROUTE_MODEL
    return ROUTE_ROLLOUT if ops.beam_supported(s, a, h, nr, not has_goal_only, w, t) else ROUTE_MODEL


def beam_host(score_fn, n, beam, horizon, n_actions):
    """The tree search on the host, the algorithm of csrc/beam.hip in numpy over score_fn(plans int32 [N,C,t+1]) -> fp32 [N,C]: the
    ret of each prefix plan (what a (t+1)-step rollout returns for it; at t + 1 = horizon the leaf's return).
    Returns a dict: best_plan int32 [N,T], best_return fp32 [N], leaf_plans int32 [N,L,T], leaf_returns fp32 [N,L], exact, expanded."""
    sizes = search_sizes(beam, horizon, n_actions)
    a = int(n_actions)
    prefixes = np.zeros((n, 1, 0), np.int32)
    for t in range(horizon):
        f = prefixes.shape[1]
        last = np.broadcast_to(np.tile(np.arange(a, dtype=np.int32), f)[None, :, None], (n, f * a, 1))
        children = np.concatenate((np.repeat(prefixes, a, axis=1), last), axis=2)  # child c = f * A + a
        ret = np.asarray(score_fn(children), np.float32).reshape(n, f * a)
        key = np.where(np.isnan(ret), np.float32(-np.inf), ret)
        if t == horizon - 1:
            break
        if f * a > beam:
            order = np.argsort(-key, axis=1, kind="stable")[:, :beam]  # key descending, ties in c ascending
            children = np.take_along_axis(children, order[:, :, None], axis=1)
        prefixes = children
    top = np.argmax(key, axis=1)  # the first maximum: ties go to the lowest c
    rows = np.arange(n)
    return dict(best_plan=children[rows, top].copy(), best_return=ret[rows, top].copy(), leaf_plans=children, leaf_returns=ret,
                exact=sizes["exact"], expanded=sizes["expanded"])


# ---- the dynamics' own metric: the k-step error on a recorded sequence (include/srlz.h states the rule) ----
HORIZON_MAX_T = 32  # steps one srlz_horizon_rows call takes


class HorizonError(object):
    """What LatentDynamics.horizon_error returns: numpy arrays per horizon [T]; a field the call has no head or no rewards for (or
    did not ask for) is None."""
    __slots__ = ("horizon", "count", "mse", "baseline_mse", "ratio", "reward_accuracy", "majority_accuracy", "err", "base", "logits",
                 "sum_err", "sum_base", "hits")

    def __init__(self, horizon, count, sum_err, sum_base, state_dim, hits=None, majority_accuracy=None, err=None, base=None, logits=None):
        self.horizon, self.count = int(horizon), np.asarray(count, np.int64)
        self.sum_err, self.sum_base = np.asarray(sum_err, np.float64), np.asarray(sum_base, np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.mse = self.sum_err / (self.count * float(state_dim))
            self.baseline_mse = self.sum_base / (self.count * float(state_dim))
            self.ratio = self.sum_err / self.sum_base
            self.hits = None if hits is None else np.asarray(hits, np.int64)
            self.reward_accuracy = None if hits is None else self.hits / self.count.astype(np.float64)
        self.majority_accuracy = majority_accuracy
        self.err, self.base, self.logits = err, base, logits

    def as_dict(self):
        """The JSON of evaluation.predict_forward: lists per horizon, None for what the call did not have; a value that is no
        finite number (a horizon no row reaches) is None too."""
        lst = lambda v: None if v is None else [float(x) if np.isfinite(x) else None for x in v]  # noqa: E731
        return {"horizon": self.horizon, "count": [int(c) for c in self.count], "mse": lst(self.mse), "baseline_mse": lst(self.baseline_mse),
                "ratio": lst(self.ratio), "reward_accuracy": lst(self.reward_accuracy), "majority_accuracy": lst(self.majority_accuracy)}


def valid_steps(episode_starts, horizon):
    """int32 [N]: for every frame i the largest L <= horizon such that frames i + 1 .. i + L exist and none of them starts an
    episode — the steps of the recorded sequence an open-loop plan from frame i may take."""
    es = np.asarray(episode_starts).reshape(-1) != 0
    t = int(horizon)
    if t < 1:
        raise ValueError("horizon must be at least 1, got %r" % (horizon,))
    n = es.shape[0]
    first = np.flatnonzero(es)  # ascending
    nxt = np.full(n, n, np.int64)  # the first episode start behind frame i, N when there is none
    if first.size:
        pos = np.searchsorted(first, np.arange(n), side="right")
        nxt = np.where(pos < first.size, first[np.minimum(pos, first.size - 1)], n)
    return np.minimum(nxt - 1 - np.arange(n), t).astype(np.int32)


def reward_classes(rewards):
    """Rewards as stored -> int64 classes, the learner's own labelling: negative rewards count as 0, then the integer cast; a class
    outside [0, 2) raises ValueError."""
    r = np.array(rewards, copy=True).reshape(-1)
    r[r < 0] = 0
    classes = r.astype(np.int64)
    if classes.size and (classes.min() < 0 or classes.max() > 1):
        raise ValueError("the reward head has two classes: after mapping -1 to 0 rewards must fall in [0, 2), found classes %s"
                         % sorted(set(classes.tolist())))
    return classes


def horizon_totals(err, base, lens, logits=None, labels=None, starts=None):
    """The per-horizon totals in numpy fp64 from rows err, base [M,T] (and logits [M,T,2] with labels [N], starts [M]):
    (count, sum_err, sum_base, hits | None).  What route "model" sums with; srlz_horizon_sums' order differs, its rule is this one."""
    err, base, lens = np.asarray(err, np.float64), np.asarray(base, np.float64), np.asarray(lens).reshape(-1)
    t = err.shape[1]
    valid = np.arange(t)[None, :] < lens[:, None]
    count = valid.sum(axis=0).astype(np.int64)
    sum_err = np.where(valid, err, 0.0).sum(axis=0)
    sum_base = np.where(valid, base, 0.0).sum(axis=0)
    hits = None
    if logits is not None:
        lg = np.asarray(logits)
        with np.errstate(invalid="ignore"):
            cls = (lg[..., 1] > lg[..., 0]).astype(np.int64)  # torch's argmax: a tie or a NaN is class 0
        frame = np.minimum(np.asarray(starts, np.int64)[:, None] + np.arange(t)[None, :], len(labels) - 1)
        hits = (valid & (cls == np.asarray(labels)[frame])).sum(axis=0).astype(np.int64)
    return count, sum_err, sum_base, hits


def majority_accuracy(labels, starts, lens, horizon):
    """fp64 [T]: per horizon the share of the commoner class among labels[starts[r] + t] over the valid (r, t) — what a constant
    answer scores.  From the labels alone."""
    t = int(horizon)
    starts, lens = np.asarray(starts, np.int64), np.asarray(lens).reshape(-1)
    valid = np.arange(t)[None, :] < lens[:, None]
    frame = np.minimum(starts[:, None] + np.arange(t)[None, :], len(labels) - 1)
    ones = (valid & (np.asarray(labels)[frame] == 1)).sum(axis=0).astype(np.float64)
    count = valid.sum(axis=0).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.maximum(ones, count - ones) / count


def check_recording(states_n, actions, episode_starts, horizon, n_actions, starts=None):
    """Validate the recorded sequence of a horizon_error call -> (actions int32 [N] on the host, starts int32 [M], lens int32 [M]).
    ValueError: lengths that disagree, non-integer actions, a start outside the sequence, no start with a valid step, an action
    outside [0, n_actions) inside a valid step."""
    n = int(states_n)
    if torch.is_tensor(actions):
        actions = actions.detach().cpu().numpy()
    actions = np.asarray(actions).reshape(-1)
    if not np.issubdtype(actions.dtype, np.integer):
        if not np.all(actions == np.floor(actions)):
            raise ValueError("actions must be integers (got %s)" % (actions.dtype,))
        actions = actions.astype(np.int64)
    if torch.is_tensor(episode_starts):
        episode_starts = episode_starts.detach().cpu().numpy()
    es = np.asarray(episode_starts).reshape(-1)
    if actions.shape[0] != n or es.shape[0] != n:
        raise ValueError("states, actions and episode_starts must have one entry per frame, got %d, %d and %d" % (n, actions.shape[0], es.shape[0]))
    lens_all = valid_steps(es, horizon)
    if starts is None:
        starts = np.flatnonzero(lens_all >= 1)
    else:
        if torch.is_tensor(starts):
            starts = starts.detach().cpu().numpy()
        starts = np.asarray(starts).reshape(-1)
        if not np.issubdtype(starts.dtype, np.integer):
            raise ValueError("starts must be integer frame indices (got %s)" % (starts.dtype,))
        if starts.size and (starts.min() < 0 or starts.max() >= n):
            raise ValueError("starts must lie in [0, %d), got %d .. %d" % (n, starts.min(), starts.max()))
    if starts.size < 1:
        raise ValueError("no start frame has a valid step: every frame is the last of its episode")
    lens = lens_all[starts]
    cover = np.zeros(n + 1, np.int64)  # frames whose action some row takes
    np.add.at(cover, starts, 1)
    np.add.at(cover, starts + lens, -1)
    used = np.cumsum(cover)[:n] > 0
    if used.any():
        lo, hi = int(actions[used].min()), int(actions[used].max())
        if lo < 0 or hi >= n_actions:
            raise ValueError("actions must lie in [0, %d) inside every valid step, got %d .. %d" % (n_actions, lo, hi))
    return np.where(used, actions, 0).astype(np.int32), starts.astype(np.int32), lens.astype(np.int32)


def horizon_route_for(model, has_reward=True, horizon=1, max_horizon=32):
    """The route LatentDynamics.horizon_error takes (host only: no GPU is asked for).  has_reward: the reward head is asked."""
    from models.modules import SRLModules
    owner = _dynamics_owner(model)
    s, a, h, nr = dynamics_dims(model)
    ok = isinstance(owner, SRLModules) and a >= 1 and owner.forward_net.bias is not None and \
        1 <= int(horizon) <= min(HORIZON_MAX_T, int(max_horizon)) and ops.horizon_supported(s, a, h, nr, has_reward)
    return ROUTE_ROLLOUT if ok else ROUTE_MODEL


def philox4x32_10(counter, key):
    """Philox4x32-10 on numpy uint64 arrays of 32-bit words: counter (c0, c1, c2, c3), key (k0, k1) -> four words."""
    lo32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = [np.asarray(c, np.uint64) for c in counter]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        a, b = c0 * np.uint64(0xD2511F53), c2 * np.uint64(0xCD9E8D57)
        c0, c1, c2, c3 = (b >> np.uint64(32)) ^ c1 ^ k0, b & lo32, (a >> np.uint64(32)) ^ c3 ^ k1, a & lo32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & lo32, (k1 + np.uint64(0xBB67AE85)) & lo32
    return c0, c1, c2, c3


def sample_actions(u, cum_row):
    """Actions of the 32-bit draws u on one table row (uint32 prefix sums): the first a with cum[a] > (u * cum[A-1]) >> 32."""
    row = np.asarray(cum_row, np.uint64)
    target = (np.asarray(u, np.uint64) * row[-1]) >> np.uint64(32)
    return np.searchsorted(row, target, side="right").astype(np.int32)


def sample_plans(cum, seed, iteration, n_plans):
    """int32 [N,K,T]: the population of one iteration from the table cum [N,T,A]."""
    n, t, _ = cum.shape
    key = (seed & 0xFFFFFFFF, seed >> 32)
    plans = np.empty((n, n_plans, t), np.int32)
    ks = np.arange(n_plans, dtype=np.uint64)
    for e in range(n):
        for t4 in range(0, t, 4):
            words = philox4x32_10((np.full_like(ks, t4 >> 2), ks, np.full_like(ks, e), np.full_like(ks, iteration)), key)
            for step in range(t4, min(t4 + 4, t)):
                plans[e, :, step] = sample_actions(words[step & 3], cum[e, step])
    return plans


def weights_of_table(cum):
    return np.diff(np.asarray(cum).astype(np.int64), axis=-1, prepend=0)


def cem_host(returns_fn, n, n_plans, horizon, n_actions, iterations, elites, sharpness, seed, init_weights=None, keep_population=False):
    """The planner on the host, the algorithm of csrc/plan.hip in numpy over returns_fn(plans int32 [N,K,T]) -> fp32 [N,K].
    Returns a dict: best_plan [N,T], best_return [N], cum uint32 [N,T,A], history [I,N] (the best key after each iteration), and with
    keep_population plans [I,N,K,T] and returns [I,N,K]."""
    if init_weights is None:
        w = np.ones((n, horizon, n_actions), np.uint64)
    else:
        w = np.broadcast_to(np.asarray(init_weights).astype(np.uint64), (n, horizon, n_actions))
    cum = np.cumsum(w, axis=2).astype(np.uint32)
    best_plan, best_return = np.zeros((n, horizon), np.int32), np.zeros(n, np.float32)
    best_key = np.full(n, -np.inf, np.float32)
    pops, rets, history = [], [], []
    steps = np.arange(horizon)
    for i in range(iterations):
        plans = sample_plans(cum, seed, i, n_plans)
        returns = np.asarray(returns_fn(plans), np.float32).reshape(n, n_plans)
        keys = np.where(np.isnan(returns), np.float32(-np.inf), returns)
        for e in range(n):
            order = np.argsort(-keys[e], kind="stable")[:elites]  # key descending, ties in k ascending
            top = order[0]
            if i == 0 or keys[e, top] > best_key[e]:
                best_key[e], best_return[e], best_plan[e] = keys[e, top], returns[e, top], plans[e, top]
            count = np.zeros((horizon, n_actions), np.uint64)
            for el in order:
                np.add.at(count, (steps, plans[e, el]), np.uint64(1))
            cum[e] = np.cumsum(np.uint64(1) + np.uint64(sharpness) * count, axis=1).astype(np.uint32)
        history.append(best_key.copy())
        if keep_population:
            pops.append(plans)
            rets.append(returns)
    out = dict(best_plan=best_plan, best_return=best_return, cum=cum, history=np.stack(history))
    if keep_population:
        out["plans"], out["returns"] = np.stack(pops), np.stack(rets)
    return out


class LatentDynamics(object):
    def __init__(self, model, max_rows=8192, max_horizon=32, untrained_ok=False, route=None):
        """model: SRLModules / SRLModulesSplit / a learner.  max_rows: N * K rows a "rollout" call may take, max_horizon: its steps;
        beyond either a call takes route "model".  untrained_ok: use heads the model's losses did not train (seeded tests).
        route="model" forces the fallback for every call (tools/kb_dynamics.py measures the two routes side by side)."""
        if route not in (None, ROUTE_MODEL):
            raise ValueError("route must be None or 'model', got %r" % (route,))
        if int(max_rows) < 1 or int(max_horizon) < 1:
            raise ValueError("max_rows and max_horizon must be at least 1, got %r and %r" % (max_rows, max_horizon))
        self.owner = _dynamics_owner(model)  # (ValueError for a model without heads, before anything touches a GPU)
        self.heads = trained_heads(model)
        self.untrained_ok = bool(untrained_ok)
        self.state_dim, self.n_actions, self._h, self._nr = dynamics_dims(model)
        picked = dynamics_route_for(model) if route is None else ROUTE_MODEL
        from models.learner import _requireGpu
        _requireGpu(True)
        self.max_rows, self.max_horizon = int(max_rows), int(max_horizon)
        self._route, self.last_route = picked, None
        self._plan_bufs = {}  # the planner's device buffers: made by the first plan call
        self._goal_bufs = {}  # the goal calls' device buffers: made by the first call with a goal
        self._search_bufs = {}  # the tree search's device buffers: made by the first search call
        self._forced_model = route is not None
        self.fit = None  # the ForwardFit of the last refit_forward / from_recording
        self.reward_fit = None  # the RewardFit of the last refit_reward / from_recording(rewards=)
        self.inverse_fit = None  # the InverseFit of the last refit_inverse / from_recording(inverse_fit=)
        self.device = next(self.owner.forward_net.parameters()).device
        if self.device.type != "cuda":
            raise C.SrlzError("LatentDynamics: the model must live on the GPU (there is no CPU path)")
        if self._route != ROUTE_ROLLOUT:
            return
        r, t, s, dev = self.max_rows, self.max_horizon, self.state_dim, self.device
        self._states = torch.empty((r, s), dtype=torch.float32, device=dev)
        self._pin_states = torch.empty((r, s), dtype=torch.float32).pin_memory()
        self._plans = torch.empty(r * t, dtype=torch.int32, device=dev)
        self._pin_plans = torch.empty(r * t, dtype=torch.int32).pin_memory()
        self._final = torch.empty(r * s, dtype=torch.float32, device=dev)
        self._returns = torch.empty(r, dtype=torch.float32, device=dev)
        self._traj = torch.empty(r * t * s, dtype=torch.float32, device=dev)
        self._logits = torch.empty(r * t * 2, dtype=torch.float32, device=dev)

    @classmethod
    def from_log_folder(cls, log_folder, max_rows=8192, max_horizon=32, valid_models=None):
        """The dynamics of a trained experiment: <log_folder>/exp_config.json + srl_model.pth (SRL4robotics.loadSavedModel)."""
        from models.learner import SRL4robotics, _requireGpu
        _requireGpu(True)
        if valid_models is None:
            valid_models = ["forward", "inverse", "reward", "priors", "episode-prior", "reward-prior", "triplet", "autoencoder", "vae",
                            "perceptual", "dae", "random"]
        if not log_folder.endswith("/"):
            log_folder += "/"
        srl, _ = SRL4robotics.loadSavedModel(log_folder, valid_models, cuda=True)
        srl.model.eval()
        return cls(srl.model, max_rows=max_rows, max_horizon=max_horizon)

    @property
    def route(self):
        """The route of the most recent call; before any call, the route that calls within max_rows and max_horizon take."""
        return self.last_route or self._route

    @classmethod
    def from_recording(cls, states, actions, episode_starts, n_actions=None, ridge=1e-6, starts=None, max_rows=8192, max_horizon=32,
                       rewards=None, reward_fit=None, inverse_fit=None):
        """Dynamics for a representation that has no network behind it (PCA, supervised or ground-truth states, a model trained
        without the forward loss): the three heads alone (srlz.dynfit.heads_only_modules, losses = ["forward"], no encoder), the
        forward head fitted to the recording in closed form (srlz.dynfit.fit_forward; the arguments are its own).  The route is the
        one a trained model of these dimensions takes.  Without `rewards` the reward head is untrained and stays unused, and goal=
        planning works on the distance term alone; with `rewards` [N] the forward fit is followed by refit_reward on the same
        transitions (reward_fit: a dict of srlz.headfit.fit_reward keyword arguments; `starts`, when given, are its training
        transitions too, and its validation transitions are then the recording's other transitions unless reward_fit names them), "reward" joins the heads and plan, search and rollout work without a goal.  The inverse head is untrained
        and stays unused with the default inverse_fit=None; with a dict of srlz.invfit.fit_inverse keyword arguments (an empty one
        for the defaults) the forward fit is followed by refit_inverse on the recording's actions, `starts` and the validation
        transitions chosen by the rule reward_fit follows; "inverse" joins the heads, and action_logits and action_accuracy work.
        The fits are kept as .fit, .reward_fit and .inverse_fit."""
        from . import dynfit
        from models.learner import _requireGpu
        if inverse_fit is not None and not isinstance(inverse_fit, dict):
            raise ValueError("inverse_fit must be None or a dict of srlz.invfit.fit_inverse keyword arguments (an empty one for the "
                             "defaults), got %s" % type(inverse_fit).__name__)
        _requireGpu(True)
        fit = dynfit.fit_forward(states, actions, episode_starts, n_actions=n_actions, ridge=ridge, starts=starts)
        model = dynfit.heads_only_modules(fit.state_dim, fit.n_actions).to(torch.device("cuda", torch.cuda.current_device()))
        model.eval()
        dyn = cls(model, max_rows=max_rows, max_horizon=max_horizon)
        dyn._install_fit(fit)

        def sides(given, name):
            kw = dict(given or {})
            if starts is not None and "starts" not in kw:
                kw["starts"] = starts
                if "val_starts" not in kw:  # the recording's other transitions: never the ones the head is trained on
                    rest = np.setdiff1d(dynfit.transitions(episode_starts), np.asarray(dynfit._host(starts)).reshape(-1))
                    if rest.size < 1:
                        raise ValueError("starts lists every transition of the recording: the %s fit has none left to pick its "
                                         "epoch on (give %s_fit=dict(val_starts=...), or fewer starts)" % (name, name))
                    kw["val_starts"] = rest.astype(np.int32)
            return kw
        if inverse_fit is not None:
            dyn.refit_inverse(states, actions, episode_starts, **sides(inverse_fit, "inverse"))
        if rewards is not None:
            dyn.refit_reward(states, rewards, episode_starts, **sides(reward_fit, "reward"))
        elif reward_fit is not None:
            raise ValueError("reward_fit configures the fit of the reward head: it needs rewards=")
        return dyn

    def _install_fit(self, fit):
        fw = self.owner.forward_net
        with torch.no_grad():
            fw.weight.copy_(torch.from_numpy(fit.weight))
            fw.bias.copy_(torch.from_numpy(fit.bias))
        if "forward" not in self.heads:
            self.heads = tuple(h for h in HEADS if h in self.heads or h == "forward")
        self.fit = fit

    def refit_forward(self, states, actions, episode_starts, ridge=1e-6, starts=None):
        """Fit the forward head to a recorded sequence in closed form (srlz.dynfit.fit_forward, n_actions = the head's) and copy the
        solution into owner.forward_net IN PLACE, under no_grad -> the ForwardFit.  "forward" joins self.heads, whatever the model's
        losses trained.  Nothing has to be refreshed: the rollout, plan, beam and horizon launches take forward_net.weight / .bias
        by address at every call and route "model" calls the owner's forwardModel, so the next call of any kind uses the new head;
        this object keeps no copy of the weights.  (A StateEncoder or FrameDecoder of the same model is not concerned: the heads
        are not theirs.)  ValueError when the recording's state_dim is not the head's, or when a listed transition holds an action
        outside the head's [0, n_actions); fit_forward's other ValueErrors as they are."""
        from . import dynfit
        if not isinstance(states, (np.ndarray, torch.Tensor)) or len(states.shape) != 2 or states.shape[1] != self.state_dim:
            raise ValueError("the recording's states of shape %s do not match the head's state_dim = %d"
                             % (tuple(getattr(states, "shape", ())), self.state_dim))
        fw = self.owner.forward_net
        if fw.bias is None:
            raise ValueError("refit_forward needs a forward head with a bias")
        fit = dynfit.fit_forward(states, actions, episode_starts, n_actions=self.n_actions, ridge=ridge, starts=starts)
        self._install_fit(fit)
        return fit

    def refit_reward(self, states, rewards, episode_starts, **fit_kwargs):
        """Train the reward head on a recorded sequence (srlz.headfit.fit_reward; hidden = the head's own H, the other keyword
        arguments are fit_reward's) and copy the kept epoch's parameters into owner.reward_net IN PLACE, under no_grad -> the
        RewardFit, kept as .reward_fit.  "reward" joins self.heads, whatever the model's losses trained.  Nothing has to be
        refreshed, for refit_forward's reason: every launch takes the head's weights by address at every call.  ValueError when the
        recording's state_dim is not the head's, when reward_net is not the reference's three-layer head with two classes
        (dynamics_dims gives H = 0), when hidden= names another width; fit_reward's ValueErrors as they are."""
        from . import headfit
        if not isinstance(states, (np.ndarray, torch.Tensor)) or len(states.shape) != 2 or states.shape[1] != self.state_dim:
            raise ValueError("the recording's states of shape %s do not match the head's state_dim = %d"
                             % (tuple(getattr(states, "shape", ())), self.state_dim))
        if self._h < 1 or self._nr != 2:
            raise ValueError("refit_reward needs the reference's reward head Linear(2S,H)-ReLU-Linear(H,H)-ReLU-Linear(H,2) with "
                             "biases; this model's reward_net is something else")
        if int(fit_kwargs.setdefault("hidden", self._h)) != self._h:
            raise ValueError("hidden=%r is not the head's own width %d" % (fit_kwargs["hidden"], self._h))
        fit = headfit.fit_reward(states, rewards, episode_starts, **fit_kwargs)
        rn = self.owner.reward_net
        with torch.no_grad():
            for key, value in fit.state_dict.items():
                layer, name = key.split(".")
                getattr(rn[int(layer)], name).copy_(value)
        if "reward" not in self.heads:
            self.heads = tuple(h for h in HEADS if h in self.heads or h == "reward")
        self.reward_fit = fit
        return fit

    def _inverse_head(self):
        """("linear" | "mlp" | None, the head's A): what owner.inverse_net is, in the words of --inverse-model-type."""
        net = getattr(self.owner, "inverse_net", None)
        s = self.state_dim
        if isinstance(net, torch.nn.Linear) and net.bias is not None and net.in_features == 2 * s:
            return "linear", net.out_features
        if isinstance(net, torch.nn.Sequential) and len(net) == 5 and all(isinstance(net[i], torch.nn.Linear) and net[i].bias is not None
                                                                          for i in (0, 2, 4)):
            from . import invfit
            h = invfit.MLP_HIDDEN
            if (net[0].in_features, net[0].out_features, net[2].in_features, net[2].out_features, net[4].in_features) == (2 * s, h, h, h, h):
                return "mlp", net[4].out_features
        return None, 0

    def refit_inverse(self, states, actions, episode_starts, **fit_kwargs):
        """Train the inverse head on a recorded sequence (srlz.invfit.fit_inverse; n_actions and inverse_model_type are the head's
        own, the other keyword arguments are fit_inverse's) and copy the kept epoch's parameters into owner.inverse_net IN PLACE,
        under no_grad -> the InverseFit, kept as .inverse_fit.  "inverse" joins self.heads, whatever the model's losses trained;
        action_logits and action_accuracy read the head at every call, nothing has to be refreshed.  A linear head within
        srlz_invfit_supported is fitted by route "kernel", an `mlp` head (H = 128) and larger shapes by route "torch".  ValueError
        when the recording's state_dim is not the head's, when inverse_net is neither of the reference's two heads, when n_actions=
        or inverse_model_type= name another head; fit_inverse's ValueErrors as they are."""
        from . import invfit
        if not isinstance(states, (np.ndarray, torch.Tensor)) or len(states.shape) != 2 or states.shape[1] != self.state_dim:
            raise ValueError("the recording's states of shape %s do not match the head's state_dim = %d"
                             % (tuple(getattr(states, "shape", ())), self.state_dim))
        kind, a = self._inverse_head()
        if kind is None:
            raise ValueError("refit_inverse needs the reference's inverse head, Linear(2S,A) or Linear(2S,128)-ReLU-Linear(128,128)-"
                             "ReLU-Linear(128,A), with biases; this model's inverse_net is something else")
        if fit_kwargs.get("n_actions") is None:
            fit_kwargs["n_actions"] = a
        if int(fit_kwargs["n_actions"]) != a:
            raise ValueError("n_actions=%r is not the head's own %d" % (fit_kwargs["n_actions"], a))
        if fit_kwargs.setdefault("inverse_model_type", kind) != kind:
            raise ValueError("inverse_model_type=%r is not the head's own %r" % (fit_kwargs["inverse_model_type"], kind))
        fit = invfit.fit_inverse(states, actions, episode_starts, **fit_kwargs)
        net = self.owner.inverse_net
        with torch.no_grad():
            for key, value in fit.state_dict.items():
                target = net
                for part in key.split("."):
                    target = target[int(part)] if part.isdigit() else getattr(target, part)
                target.copy_(value)
        if "inverse" not in self.heads:
            self.heads = tuple(h for h in HEADS if h in self.heads or h == "inverse")
        self.inverse_fit = fit
        return fit

    def action_accuracy(self, states, actions, episode_starts, starts=None):
        """How well the inverse head reads the recorded action off (states[i], states[i + 1]) -> ActionAccuracy: count, accuracy,
        majority_accuracy (the share of the most frequent action: what a constant answer scores), recall / support / hits per action
        (recall None for an action without a row), loss (the mean cross-entropy), route.  The transitions are `starts`, or every
        frame whose successor belongs to its episode.  Needs a trained or fitted inverse head (the gating ValueError of
        action_logits).  A linear head of SRLModules within srlz_invfit_supported is ONE srlz_invfit_eval launch (route "kernel");
        anything else goes through the model's own inverseModel in batches of max_rows (route "model"), counted on the device.  An
        argmax tie goes to the lowest action."""
        from . import dynfit
        from models.modules import SRLModules
        self._need("inverse")
        if not isinstance(states, (np.ndarray, torch.Tensor)) or len(states.shape) != 2 or states.shape[1] != self.state_dim:
            raise ValueError("the recording's states of shape %s do not match the head's state_dim = %d"
                             % (tuple(getattr(states, "shape", ())), self.state_dim))
        kind, a = self._inverse_head()
        if kind is None:
            a = self.n_actions
        labels, starts, _ = dynfit.check_fit_recording(states, actions, episode_starts, n_actions=a, starts=starts)
        n, s = int(states.shape[0]), self.state_dim
        x = self._device_states(states, n, False, False)
        d_labels = torch.from_numpy(labels).to(self.device)
        counts = torch.zeros(ops.invfit_n_counts(a), dtype=torch.int64, device=self.device)
        loss = torch.zeros(1, dtype=torch.float64, device=self.device)
        kernel = kind == "linear" and isinstance(self.owner, SRLModules) and not self._forced_model and ops.invfit_supported(s, a) \
            and n * s < 2 ** 31
        if kernel:
            net = self.owner.inverse_net
            with torch.no_grad():
                flat = torch.cat((net.weight.detach().reshape(-1), net.bias.detach().reshape(-1))).float().contiguous()
            ops.invfit_eval(ops.RewardProbeData(x, d_labels), torch.from_numpy(starts.reshape(1, -1)), a, flat, loss, counts)
        else:
            from . import invfit
            d_starts = torch.from_numpy(starts).to(self.device).long()
            with torch.no_grad():
                for lo in range(0, d_starts.shape[0], self.max_rows):
                    i = d_starts[lo:lo + self.max_rows]
                    z, y = self.owner.inverseModel(x[i], x[i + 1]), d_labels[i].long()
                    loss += torch.nn.functional.cross_entropy(z.double(), y, reduction="sum")
                    counts += invfit._torch_counts(z, y, a)
        c = counts.cpu().numpy()
        return ActionAccuracy(c, float(loss.cpu()[0]), a, "kernel" if kernel else ROUTE_MODEL)

    def _need(self, head):
        if head in self.heads:  # (refit_forward / refit_reward / refit_inverse add their head to the heads the losses trained)
            return
        check_head(self.owner, head, self.untrained_ok)

    def _uses_reward(self):
        return self.untrained_ok or "reward" in self.heads

    # ---------------------------------------------------------------------------------------------------------
    def _device_states(self, states, n, single, staged):
        """The call's states as a contiguous fp32 device tensor [n, S]: the caller's own when it already is one, else (staged) a copy
        into the staging buffer (host states travel through the pinned one), else a fresh tensor."""
        if isinstance(states, np.ndarray):
            states = torch.from_numpy(np.ascontiguousarray(states))
        states = states.detach()
        if single:
            states = states.unsqueeze(0)
        if states.device.type == "cuda" and states.is_contiguous() and states.dtype == torch.float32:
            return states
        if not staged:
            return states.to(self.device, torch.float32).contiguous()
        if states.device.type == "cuda":
            self._states[:n].copy_(states)
        else:
            self._pin_states[:n].copy_(states)
            self._states[:n].copy_(self._pin_states[:n], non_blocking=True)
        return self._states[:n]

    def _device_plans(self, plans, shape, staged):
        """The call's plans on the device with `shape` ([N,K,T] or [K,T]): int32 in the staging buffer (staged), else int64."""
        if isinstance(plans, np.ndarray):
            plans = torch.from_numpy(np.ascontiguousarray(plans))
        plans = plans.reshape(shape)
        if not staged:
            return plans.to(self.device, torch.int64).contiguous()
        if plans.device.type == "cuda" and plans.dtype == torch.int32 and plans.is_contiguous():
            return plans
        numel = plans.numel()
        dst = self._plans[:numel].view(shape)
        if plans.device.type == "cuda":
            dst.copy_(plans)
        else:
            pin = self._pin_plans[:numel].view(shape)
            pin.copy_(plans)
            dst.copy_(pin, non_blocking=True)
        return dst

    def _model_rollout(self, states, plans, gamma, reward, keep_trajectory, keep_logits):
        """Route "model": the owner's own forwardModel and rewardModel, step by step, under no_grad.  states [n,S] fp32, plans int64
        [n,k,t] or [k,t] on the device."""
        n, s = states.shape
        if plans.dim() == 2:
            plans = plans.unsqueeze(0).expand(n, -1, -1)
        k, t = plans.shape[1], plans.shape[2]
        acts = plans.reshape(n * k, t)
        traj, logits = [], []
        with torch.no_grad():
            cur = states.unsqueeze(1).expand(n, k, s).reshape(n * k, s).contiguous()
            ret = torch.zeros(n * k, dtype=torch.float32, device=states.device) if reward else None
            g = torch.ones((), dtype=torch.float32, device=states.device)
            for step in range(t):
                nxt = self.owner.forwardModel(cur, acts[:, step].contiguous())
                if keep_trajectory:
                    traj.append(nxt)
                if reward:
                    lg = self.owner.rewardModel(cur, nxt)
                    if keep_logits:
                        logits.append(lg)
                    ret = ret + g * torch.softmax(lg, dim=1)[:, 1]
                    g = g * gamma
                cur = nxt
        return (cur.view(n, k, s), ret.view(n, k) if reward else None,
                torch.stack(traj, dim=1).view(n, k, t, s) if keep_trajectory else None,
                torch.stack(logits, dim=1).view(n, k, t, 2) if keep_logits else None)

    def _run(self, states, plans, gamma, reward, keep_trajectory, keep_logits):
        """Both routes on checked inputs -> (final [n,k,S], returns [n,k] | None, trajectory | None, logits | None, plans on the device,
        single, bare)."""
        n, single = check_states(states, self.state_dim)
        k, t, shared, bare = check_plans(plans, n, self.n_actions)
        shape = (k, t) if shared else (n, k, t)
        staged = self._route == ROUTE_ROLLOUT and n * k <= self.max_rows and t <= self.max_horizon
        self.last_route = ROUTE_ROLLOUT if staged else ROUTE_MODEL
        x = self._device_states(states, n, single, staged)
        pl = self._device_plans(plans, shape, staged)
        if not staged:
            return self._model_rollout(x, pl, gamma, reward, keep_trajectory, keep_logits) + (pl, single, bare)
        s, o = self.state_dim, self.owner
        final = self._final[:n * k * s].view(n, k, s)
        returns = self._returns[:n * k].view(n, k) if reward else None
        traj = self._traj[:n * k * t * s].view(n, k, t, s) if keep_trajectory else None
        logits = self._logits[:n * k * t * 2].view(n, k, t, 2) if keep_logits else None
        rn = o.reward_net
        head = (rn[0].weight, rn[0].bias, rn[2].weight, rn[2].bias, rn[4].weight, rn[4].bias) if reward else None
        ops.rollout(x, pl, o.forward_net.weight, o.forward_net.bias, reward=head, final=final, returns=returns, trajectory=traj,
                    reward_logits=logits, gamma=gamma)
        return final, returns, traj, logits, pl, single, bare

    # ---- calls with a goal (a call without one never comes here) ----
    def _goal_reward(self):
        """Whether the reward head joins a goal call's score: a trained one does, an untrained one only under untrained_ok."""
        return self._uses_reward()

    def _goal_kernel_ok(self, reward):
        return not self._forced_model and goal_route_for(self.owner, not reward) == ROUTE_ROLLOUT

    def _goal_buffers(self, n):
        """The staging buffers of a "rollout" call with a goal: the constructor's when it made them (a goal-only call can take the
        kernel where the reward head's shape refused it), the goal and goal_dist buffers; made once, grown never (n <= max_rows)."""
        r, t, s, dev = self.max_rows, self.max_horizon, self.state_dim, self.device
        if not hasattr(self, "_states"):
            self._states = torch.empty((r, s), dtype=torch.float32, device=dev)
            self._pin_states = torch.empty((r, s), dtype=torch.float32).pin_memory()
            self._plans = torch.empty(r * t, dtype=torch.int32, device=dev)
            self._pin_plans = torch.empty(r * t, dtype=torch.int32).pin_memory()
            self._final = torch.empty(r * s, dtype=torch.float32, device=dev)
            self._returns = torch.empty(r, dtype=torch.float32, device=dev)
            self._traj = torch.empty(r * t * s, dtype=torch.float32, device=dev)
            self._logits = torch.empty(r * t * 2, dtype=torch.float32, device=dev)
        b = self._goal_bufs
        if not b:
            b["goal"] = torch.empty((r, s), dtype=torch.float32, device=dev)
            b["dist"] = torch.empty(r * t, dtype=torch.float32, device=dev)
        return b

    def _device_goal(self, goal, shared, n, staged):
        """The call's goal as a contiguous fp32 device tensor [S] or [n,S]: the caller's own when it already is one, else a copy (into
        the goal buffer when staged)."""
        if isinstance(goal, np.ndarray):
            goal = torch.from_numpy(np.ascontiguousarray(goal))
        goal = goal.detach()
        if goal.device.type == "cuda" and goal.is_contiguous() and goal.dtype == torch.float32:
            return goal
        if not staged:
            return goal.to(self.device, torch.float32).contiguous()
        dst = self._goal_bufs["goal"][0] if shared else self._goal_bufs["goal"][:n]
        dst.copy_(goal, non_blocking=True)
        return dst

    def _model_rollout_goal(self, states, plans, goal, gamma, weight, mode, reward, keep_logits):
        """Route "model" with a goal: the owner's own forwardModel and rewardModel step by step, scored by goal_scores."""
        final, _, traj, logits = self._model_rollout(states, plans, gamma, False, True, False)
        n, k, t, s = traj.shape
        probs = lg = None
        if reward:
            with torch.no_grad():
                prev = torch.cat((states.view(n, 1, 1, s).expand(n, k, 1, s), traj[:, :, :-1]), dim=2).reshape(-1, s)
                lg = self.owner.rewardModel(prev, traj.reshape(-1, s)).view(n, k, t, 2)
                probs = torch.softmax(lg, dim=-1)[..., 1]
        scores, dist = goal_scores(traj, goal, probs, gamma, weight, mode)
        return final, scores, traj, (lg if keep_logits else None), dist

    def _run_goal(self, states, plans, goal, gamma, weight, mode, reward, keep_trajectory, keep_logits, keep_dist):
        """Both routes on checked inputs, with a goal -> (final [n,k,S], scores [n,k], trajectory | None, logits | None,
        goal_dist | None, plans on the device, single, bare)."""
        n, single = check_states(states, self.state_dim)
        k, t, shared, bare = check_plans(plans, n, self.n_actions)
        goal_shared = check_goal(goal, n, self.state_dim)
        shape = (k, t) if shared else (n, k, t)
        staged = self._goal_kernel_ok(reward) and n * k <= self.max_rows and t <= self.max_horizon
        self.last_route = ROUTE_ROLLOUT if staged else ROUTE_MODEL
        if staged:
            b = self._goal_buffers(n)
        x = self._device_states(states, n, single, staged)
        pl = self._device_plans(plans, shape, staged)
        gl = self._device_goal(goal, goal_shared, n, staged)
        if not staged:
            final, scores, traj, logits, dist = self._model_rollout_goal(x, pl, gl, gamma, weight, mode, reward, keep_logits)
            return final, scores, (traj if keep_trajectory else None), logits, (dist if keep_dist else None), pl, single, bare
        s, o = self.state_dim, self.owner
        final = self._final[:n * k * s].view(n, k, s)
        scores = self._returns[:n * k].view(n, k)
        traj = self._traj[:n * k * t * s].view(n, k, t, s) if keep_trajectory else None
        logits = self._logits[:n * k * t * 2].view(n, k, t, 2) if keep_logits else None
        dist = b["dist"][:n * k * t].view(n, k, t) if keep_dist else None
        rn = o.reward_net
        head = (rn[0].weight, rn[0].bias, rn[2].weight, rn[2].bias, rn[4].weight, rn[4].bias) if reward else None
        ops.rollout_goal(x, pl, o.forward_net.weight, o.forward_net.bias, gl, reward=head, final=final, returns=scores, trajectory=traj,
                         reward_logits=logits, goal_dist=dist, gamma=gamma, goal_weight=weight, goal_mode=mode)
        return final, scores, traj, logits, dist, pl, single, bare

    @staticmethod
    def _best(returns):
        """argmax_k of returns [n,k], ties to the lowest k (torch.argmax returns the first maximal value); a NaN return is never
        chosen over a number."""
        return torch.nan_to_num(returns, nan=float("-inf")).argmax(dim=1)

    @staticmethod
    def _drop(x, single, bare, k_axis=1):
        """Drop the axes the inputs did not have: K (a bare [T] plan) first, then N (a bare [S] state)."""
        if x is None:
            return None
        if bare and x.dim() > k_axis:
            x = x.squeeze(k_axis)
        return x[0] if single else x

    def rollout(self, states, plans, gamma=1.0, keep_trajectory=False, keep_logits=False, goal=None, goal_weight=1.0,
                goal_mode="running", keep_goal_dist=False):
        self._need("forward")
        reward = self._uses_reward()
        if keep_logits and not reward:
            self._need("reward")
        if goal is not None:  # returns is the score (include/srlz.h), with or without a reward head
            w, mode = check_goal_args(goal_weight, goal_mode)
            final, scores, traj, logits, dist, _, single, bare = self._run_goal(states, plans, goal, float(gamma), w, mode, reward,
                                                                                keep_trajectory, keep_logits, keep_goal_dist)
            best = self._best(scores)
            d = self._drop
            return Rollout(d(final, single, bare), d(scores, single, bare), d(traj, single, bare), d(logits, single, bare),
                           best[0] if single else best, d(dist, single, bare))
        if keep_goal_dist:
            raise ValueError("keep_goal_dist needs a goal")
        final, returns, traj, logits, _, single, bare = self._run(states, plans, float(gamma), reward, keep_trajectory, keep_logits)
        best = self._best(returns) if reward else None
        d = self._drop
        return Rollout(d(final, single, bare), d(returns, single, bare), d(traj, single, bare), d(logits, single, bare),
                       best[0] if best is not None and single else best)

    def step(self, states, actions):
        """[N,S], [N] -> [N,S] (one bare state and one action: [S]): forwardModel alone, the same kernel with K = T = 1."""
        self._need("forward")
        n, single = check_states(states, self.state_dim)
        if not isinstance(actions, (np.ndarray, torch.Tensor)):
            actions = np.asarray(actions)
        if tuple(actions.shape) != (() if single else (n,)):
            raise ValueError("actions of shape %s do not match %d states" % (tuple(actions.shape), n))
        final = self._run(states, actions.reshape(n, 1, 1), 1.0, False, False, False)[0]
        return final[0, 0] if single else final[:, 0]

    def act(self, states, plans, goal=None, goal_weight=1.0, goal_mode="running"):
        """First action of each environment's best plan: [N] int64 ([] for one bare state), computed on the device.  With a goal the
        plans are ranked by the score and only the forward head is required."""
        self._need("forward")
        if goal is not None:
            w, mode = check_goal_args(goal_weight, goal_mode)
            _, returns, _, _, _, pl, single, _ = self._run_goal(states, plans, goal, 1.0, w, mode, self._goal_reward(), False, False,
                                                                False)
        else:
            self._need("reward")
            _, returns, _, _, pl, single, _ = self._run(states, plans, 1.0, True, False, False)
        best = self._best(returns)
        first = pl[..., 0].to(torch.int64)  # [n,k] or (shared) [k]
        a = first[best] if first.dim() == 1 else first.gather(1, best.unsqueeze(1)).squeeze(1)
        return a[0] if single else a

    def _plan_buffers(self, n, k, t, iterations, keep):
        """The planner's device buffers, made on the first plan call and grown only when a call asks for more."""
        a = self.n_actions
        want = dict(best=n * t, ret=n, cum=n * t * a, ws=ops.plan_workspace(n, k, t, keep), pop=iterations * n * k * t if keep else 0,
                    pret=iterations * n * k if keep else 0, init=n * t * a, w=n * t * a, act=n)
        kinds = dict(best=torch.int32, ret=torch.float32, cum=torch.int32, ws=torch.uint8, pop=torch.int32, pret=torch.float32,
                     init=torch.int32, w=torch.int32, act=torch.int64)
        have = self._plan_bufs
        for name, numel in want.items():
            if name not in have or have[name].numel() < numel:
                have[name] = torch.empty(max(numel, 1), dtype=kinds[name], device=self.device)
        return have

    def plan(self, states, horizon, n_plans=64, iterations=4, elites=8, sharpness=8, gamma=1.0, seed=0, init_weights=None,
             keep_population=False, goal=None, goal_weight=1.0, goal_mode="running"):
        """A categorical cross-entropy search for each environment's action sequence (the comment block above states it) -> Plan.
        With a goal the plans are keyed by the score (best_return and returns are scores) and only the forward head is required."""
        self._need("forward")
        if goal is None:
            self._need("reward")
        n, single = check_states(states, self.state_dim)
        t, k, it, e, q, seed = check_plan_args(horizon, n_plans, iterations, elites, sharpness, seed)
        init_weights, shared = check_init_weights(init_weights, n, t, self.n_actions)
        a = self.n_actions
        if goal is None:
            kernel = self._route == ROUTE_ROLLOUT and n * k <= self.max_rows and \
                ops.plan_supported(self.state_dim, a, self._h, self._nr, k, t)
        else:
            goal_shared = check_goal(goal, n, self.state_dim)
            gw, gmode = check_goal_args(goal_weight, goal_mode)
            reward = self._goal_reward()
            kernel = self._goal_kernel_ok(reward) and n * k <= self.max_rows and \
                ops.plan_goal_supported(self.state_dim, a, self._h, self._nr, reward, k, t)
        if not kernel:
            host_w = init_weights.cpu().numpy() if torch.is_tensor(init_weights) else init_weights

            def returns_fn(pl):
                if goal is not None:
                    return self._run_goal(states, pl[0] if single else pl, goal, float(gamma), gw, gmode, reward, False, False,
                                          False)[1].reshape(n, k).float().cpu().numpy()
                return self._run(states, pl[0] if single else pl, float(gamma), True, False, False)[1].reshape(n, k).cpu().numpy()
            out = cem_host(returns_fn, n, k, t, a, it, e, q, seed, host_w, keep_population)
            self.last_route = ROUTE_MODEL
            dev = self.device
            best_plan = torch.from_numpy(out["best_plan"]).to(dev)
            best_return = torch.from_numpy(out["best_return"]).to(dev)
            weights = torch.from_numpy(weights_of_table(out["cum"]).astype(np.int32)).to(dev)
            plans = torch.from_numpy(out["plans"]).to(dev) if keep_population else None
            returns = torch.from_numpy(out["returns"]).to(dev) if keep_population else None
        else:
            self.last_route = ROUTE_ROLLOUT
            if goal is not None:
                self._goal_buffers(n)
                gl = self._device_goal(goal, goal_shared, n, True)
            x = self._device_states(states, n, single, True)
            b = self._plan_buffers(n, k, t, it, keep_population)
            iw = None
            if init_weights is not None:
                shape = (t, a) if shared else (n, t, a)
                iw = b["init"][:int(np.prod(shape))].view(shape)
                iw.copy_(torch.from_numpy(init_weights.astype(np.int32)) if isinstance(init_weights, np.ndarray) else init_weights,
                         non_blocking=True)
            best_plan, best_return = b["best"][:n * t].view(n, t), b["ret"][:n]
            cum = b["cum"][:n * t * a].view(n, t, a)
            plans = b["pop"][:it * n * k * t].view(it, n, k, t) if keep_population else None
            returns = b["pret"][:it * n * k].view(it, n, k) if keep_population else None
            o, rn = self.owner, self.owner.reward_net
            if goal is None or reward:
                head = (rn[0].weight, rn[0].bias, rn[2].weight, rn[2].bias, rn[4].weight, rn[4].bias)
            if goal is None:
                ops.plan_cem(x, o.forward_net.weight, o.forward_net.bias, head, k, t, it, e, q, best_plan, best_return, cum, b["ws"],
                             gamma=gamma, seed=seed, init_weights=iw, plans=plans, returns=returns)
            else:
                ops.plan_cem_goal(x, o.forward_net.weight, o.forward_net.bias, head if reward else None, gl, k, t, it, e, q, best_plan,
                                  best_return, cum, b["ws"], gamma=gamma, seed=seed, init_weights=iw, plans=plans, returns=returns,
                                  goal_weight=gw, goal_mode=gmode)
            weights = b["w"][:n * t * a].view(n, t, a)  # (the table's uint32 stay below 2^31 at these limits)
            weights[:, :, :1].copy_(cum[:, :, :1])
            if a > 1:
                torch.sub(cum[:, :, 1:], cum[:, :, :-1], out=weights[:, :, 1:])
            action = b["act"][:n]
            action.copy_(best_plan[:, 0])
        if not kernel:
            action = best_plan[:, 0].to(torch.int64)
        if single:
            best_plan, best_return, action, weights = best_plan[0], best_return[0], action[0], weights[0]
            plans = plans[:, 0] if plans is not None else None
            returns = returns[:, 0] if returns is not None else None
        return Plan(best_plan, best_return, action, weights, plans, returns)

    # ---- tree search ----
    def _search_buffers(self, n, w, t, leaves, keep):
        """The search's device buffers, made on the first search call and grown only when a call asks for more."""
        want = dict(best=n * t, ret=n, act=n, ws=ops.beam_workspace(n, w, t, self.state_dim, self.n_actions),
                    lp=n * leaves * t if keep else 0, lr=n * leaves if keep else 0)
        kinds = dict(best=torch.int32, ret=torch.float32, act=torch.int64, ws=torch.uint8, lp=torch.int32, lr=torch.float32)
        have = self._search_bufs
        for name, numel in want.items():
            if name not in have or have[name].numel() < numel:
                have[name] = torch.empty(max(numel, 1), dtype=kinds[name], device=self.device)
        return have

    def search(self, states, horizon, beam=64, gamma=1.0, keep_leaves=False, goal=None, goal_weight=1.0, goal_mode="running"):
        """Exact or beam tree search for each environment's action sequence (the comment block above states it) -> Search.
        With a goal the nodes are keyed by the score (best_return and leaf_returns are scores) and only the forward head is required."""
        self._need("forward")
        if goal is None:
            self._need("reward")
        n, single = check_states(states, self.state_dim)
        t, w = check_search_args(horizon, beam)
        a = self.n_actions
        reward = True
        if goal is not None:
            goal_shared = check_goal(goal, n, self.state_dim)
            gw, gmode = check_goal_args(goal_weight, goal_mode)
            reward = self._goal_reward()
        kernel = not self._forced_model and (goal is not None or self._route == ROUTE_ROLLOUT) and \
            search_route_for(self.owner, w, t, n, self.max_rows, has_goal_only=not reward) == ROUTE_ROLLOUT
        sizes = search_sizes(w, t, a)
        leaves = sizes["leaves"]
        if not kernel:
            def score_fn(pl):
                shape, arg = (n, pl.shape[1]), (pl[0] if single else pl)
                if goal is None:
                    r = self._run(states, arg, float(gamma), True, False, False)[1]
                elif gmode == "running" or pl.shape[2] == t:
                    r = self._run_goal(states, arg, goal, float(gamma), gw, gmode, reward, False, False, False)[1]
                elif reward:  # (goal mode final: the distance enters at the last level alone)
                    r = self._run(states, arg, float(gamma), True, False, False)[1]
                else:
                    return np.zeros(shape, np.float32)
                return r.reshape(shape).float().cpu().numpy()
            out = beam_host(score_fn, n, w, t, a)
            self.last_route = ROUTE_MODEL
            dev = self.device
            best_plan = torch.from_numpy(out["best_plan"]).to(dev)
            best_return = torch.from_numpy(out["best_return"]).to(dev)
            action = best_plan[:, 0].to(torch.int64)
            leaf_plans = torch.from_numpy(np.ascontiguousarray(out["leaf_plans"])).to(dev) if keep_leaves else None
            leaf_returns = torch.from_numpy(np.ascontiguousarray(out["leaf_returns"])).to(dev) if keep_leaves else None
        else:
            self.last_route = ROUTE_ROLLOUT
            w = max(sizes["frontier"])  # (a wider beam never prunes more: the same search)
            gl = None
            if goal is not None:
                self._goal_buffers(n)
                gl = self._device_goal(goal, goal_shared, n, True)
            x = self._device_states(states, n, single, True)
            b = self._search_buffers(n, w, t, leaves, keep_leaves)
            best_plan, best_return = b["best"][:n * t].view(n, t), b["ret"][:n]
            leaf_plans = b["lp"][:n * leaves * t].view(n, leaves, t) if keep_leaves else None
            leaf_returns = b["lr"][:n * leaves].view(n, leaves) if keep_leaves else None
            o, rn = self.owner, self.owner.reward_net
            head = (rn[0].weight, rn[0].bias, rn[2].weight, rn[2].bias, rn[4].weight, rn[4].bias) if reward else None
            ops.beam_search(x, o.forward_net.weight, o.forward_net.bias, head, w, t, best_plan, best_return, b["ws"], gamma=gamma,
                            leaf_plans=leaf_plans, leaf_returns=leaf_returns, goal=gl, goal_weight=gw if goal is not None else 1.0,
                            goal_mode=gmode if goal is not None else "running")
            action = b["act"][:n]
            action.copy_(best_plan[:, 0])
        if single:
            best_plan, best_return, action = best_plan[0], best_return[0], action[0]
            leaf_plans = leaf_plans[0] if leaf_plans is not None else None
            leaf_returns = leaf_returns[0] if leaf_returns is not None else None
        return Search(best_plan, best_return, action, sizes["exact"], sizes["expanded"], leaves, leaf_plans, leaf_returns)

    # ---- the k-step error on a recorded sequence ----
    def _model_horizon(self, x, acts, starts, lens, t, reward):
        """Route "model": the owner's own forwardModel / rewardModel step by step -> rows err, base fp32 [M,T] (NaN past a row's
        steps) and logits [M,T,2] | None, on the device."""
        n = x.shape[0]
        nanv = torch.tensor(float("nan"), dtype=torch.float32, device=x.device)
        errs, bases, logits = [], [], []
        with torch.no_grad():
            s0 = x[starts]
            cur = s0
            for step in range(t):
                has = lens > step
                frame = torch.clamp(starts + step, max=n - 1)
                a = torch.where(has, acts[frame], torch.zeros_like(frame))
                nxt = self.owner.forwardModel(cur, a.contiguous())
                tgt = x[torch.clamp(starts + step + 1, max=n - 1)]
                e = (nxt - tgt).double().pow(2).sum(dim=1).float()
                b = (s0 - tgt).double().pow(2).sum(dim=1).float()
                errs.append(torch.where(has, e, nanv))
                bases.append(torch.where(has, b, nanv))
                if reward:
                    logits.append(self.owner.rewardModel(cur, nxt))
                cur = nxt
        return torch.stack(errs, dim=1), torch.stack(bases, dim=1), torch.stack(logits, dim=1) if reward else None

    def horizon_error(self, states, actions, episode_starts, horizon, rewards=None, starts=None, keep_rows=False):
        """The k-step error of the forward head on a recorded sequence -> HorizonError (the section comment above states the rule).
        states [N,S] floating point (numpy or a device tensor), actions and episode_starts [N], rewards [N] as stored or None,
        starts: frame indices [M] or None (every frame with a valid step)."""
        self._need("forward")
        n, single = check_states(states, self.state_dim)
        if single:
            raise ValueError("horizon_error takes a recorded sequence [N,S], got one bare state")
        t = int(horizon)
        acts, st, ln = check_recording(n, actions, episode_starts, t, self.n_actions, starts)
        labels = None if rewards is None else reward_classes(rewards)
        if labels is not None and labels.shape[0] != n:
            raise ValueError("rewards must have one entry per frame, got %d for %d states" % (labels.shape[0], n))
        reward = labels is not None and self._uses_reward()
        kernel = not self._forced_model and horizon_route_for(self.owner, reward, t, self.max_horizon) == ROUTE_ROLLOUT
        self.last_route = ROUTE_ROLLOUT if kernel else ROUTE_MODEL
        dev = self.device
        x = self._device_states(states, n, False, False)
        d_acts = torch.from_numpy(acts).to(dev)
        d_st, d_ln = torch.from_numpy(st).to(dev), torch.from_numpy(ln).to(dev)
        m = st.shape[0]
        if kernel:
            o = self.owner
            err = torch.empty((m, t), dtype=torch.float32, device=dev)
            base = torch.empty((m, t), dtype=torch.float32, device=dev)
            logits = torch.empty((m, t, 2), dtype=torch.float32, device=dev) if reward else None
            rn = o.reward_net
            head = (rn[0].weight, rn[0].bias, rn[2].weight, rn[2].bias, rn[4].weight, rn[4].bias) if reward else None
            ops.horizon_rows(x, d_acts, d_st, d_ln, o.forward_net.weight, o.forward_net.bias, err, base, t, reward=head,
                             reward_logits=logits)
            count = torch.empty(t, dtype=torch.int64, device=dev)
            sum_err = torch.empty(t, dtype=torch.float64, device=dev)
            sum_base = torch.empty(t, dtype=torch.float64, device=dev)
            hits = torch.empty(t, dtype=torch.int64, device=dev) if reward else None
            d_lab = torch.from_numpy(labels.astype(np.int32)).to(dev) if reward else None
            ops.horizon_sums(err, base, d_st, d_ln, count, sum_err, sum_base, reward_logits=logits, labels=d_lab, hits=hits)
            count, sum_err, sum_base = count.cpu().numpy(), sum_err.cpu().numpy(), sum_base.cpu().numpy()
            hits = hits.cpu().numpy() if reward else None
        else:
            err, base, logits = self._model_horizon(x, d_acts.long(), d_st.long(), d_ln.long(), t, reward)
            count, sum_err, sum_base, hits = horizon_totals(err.cpu().numpy(), base.cpu().numpy(), ln,
                                                            logits.cpu().numpy() if reward else None, labels, st)
        major = majority_accuracy(labels, st, ln, t) if reward else None
        rows = (err, base, logits) if keep_rows else (None, None, None)
        return HorizonError(t, count, sum_err, sum_base, self.state_dim, hits, major, *rows)

    def _pair(self, states, next_states):
        n, single = check_states(states, self.state_dim)
        if check_states(next_states, self.state_dim) != (n, single):
            raise ValueError("states and next_states must have the same shape")
        return self._device_states(states, n, single, False), self._device_states(next_states, n, single, False), single

    def reward_logits(self, states, next_states):
        """The model's own rewardModel under no_grad: [N,2] ([2] for bare states)."""
        self._need("reward")
        a, b, single = self._pair(states, next_states)
        with torch.no_grad():
            out = self.owner.rewardModel(a, b)
        return out[0] if single else out

    def action_logits(self, states, next_states):
        """The model's own inverseModel under no_grad: [N,A] ([A] for bare states)."""
        self._need("inverse")
        a, b, single = self._pair(states, next_states)
        with torch.no_grad():
            out = self.owner.inverseModel(a, b)
        return out[0] if single else out


def imagine(dynamics, decoder, states, plans):
    """The imagined camera frames of every plan: the rollout's trajectory through a FrameDecoder, chunked by its max_batch so that
    every chunk takes its "blocks" route.  uint8 [N,K,T] + the decoder's frame shape (axes the inputs did not have are dropped);
    bit-identical to decoder(trajectory rows)."""
    traj = dynamics.rollout(states, plans, keep_trajectory=True).trajectory
    rows = traj.reshape(-1, traj.shape[-1])
    frames, m = None, decoder.max_batch
    for lo in range(0, rows.shape[0], m):
        part = decoder(rows[lo:lo + m])
        if frames is None:
            frames = torch.empty((rows.shape[0],) + tuple(part.shape[1:]), dtype=part.dtype, device=part.device)
        frames[lo:lo + part.shape[0]].copy_(part)
    return frames.view(tuple(traj.shape[:-1]) + tuple(frames.shape[1:]))


def reach(encoder, dynamics, frames, goal_frames, horizon, planner="cem", **plan_kwargs):
    """Plan from camera frames towards goal pictures: dynamics.plan(encoder(frames), horizon, goal=encoder(goal_frames), ...) -> Plan,
    or with planner="search" dynamics.search(...) with the same goal -> Search; the states never leaving the device.  frames and goal_frames of the same shape ([N, ...] or one bare frame each); when both fit
    the encoder's max_batch they go through it as ONE call, otherwise as two."""
    n, single = check_frames(frames, encoder.frame_layout, encoder.channels, encoder.frame_size)
    if check_frames(goal_frames, encoder.frame_layout, encoder.channels, encoder.frame_size) != (n, single):
        raise ValueError("frames and goal_frames must have the same shape, got %s and %s" % (tuple(frames.shape), tuple(goal_frames.shape)))
    if "goal" in plan_kwargs:
        raise ValueError("reach takes the goal as goal_frames")
    if planner not in ("cem", "search"):
        raise ValueError("planner must be 'cem' or 'search', got %r" % (planner,))
    # Host frames are uploaded here, with a copy that has ended when it returns: the encoder's pinned staging buffer is refilled by
    # the host at every call, and two calls back to back would refill it while the first call's copy to the device may still wait
    # on the stream.  A device tensor is read by the encoder in place.
    dev = [(torch.from_numpy(np.ascontiguousarray(f)) if isinstance(f, np.ndarray) else f).to(encoder.device) for f in (frames, goal_frames)]
    if 2 * n <= encoder.max_batch:
        both = encoder(torch.cat([f.unsqueeze(0) if single else f for f in dev], dim=0))
        states, goals = (both[0], both[1]) if single else (both[:n], both[n:])
    else:
        states = encoder(dev[0].contiguous()).clone()  # (the encoder's state buffer is reused by the next call)
        goals = encoder(dev[1].contiguous())
    if planner == "search":
        return dynamics.search(states, horizon, goal=goals, **plan_kwargs)
    return dynamics.plan(states, horizon, goal=goals, **plan_kwargs)
