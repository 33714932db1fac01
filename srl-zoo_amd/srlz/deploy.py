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
