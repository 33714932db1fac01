"""Look at a learned representation: move one latent coordinate and see what the decoder draws, or — for a model without a decoder —
which training frame lies nearest (reference evaluation/enjoy_latent.py).

    python -m evaluation.enjoy_latent --log-dir logs/<dataset>/<experiment>/                      # the reference's cv2 windows
    python -m evaluation.enjoy_latent --log-dir logs/<dataset>/<experiment>/ --sheet-dir out      # headless: traversal sheets (PNG)

The reference's command line, windows, sliders and arithmetic, quirks included:
  * one figure per sized block of `split-dimensions`, otherwise ONE figure named after losses[0], which alone decides between the
    decoder and the nearest-frame lookup;
  * the lookup is KNeighborsClassifier().fit(X, arange(N)).predict: with N different labels that is the SMALLEST INDEX among the five
    nearest rows, not the nearest row (knnImageIndex, on the exact fp64 search of srlz.ops.knn);
  * the model is never put in eval mode: every tick decodes ONE state with the decoder's BatchNorm on the statistics of that one
    image (--batchnorm reference, the default).  --batchnorm running is the intended behaviour: eval mode, running statistics.
  * a decoder with other than 3 channels (--multi-view) trips deNormalize's assertion.

What differs is where the work runs: the decoded tensor becomes the BGR image (or, headless, a whole sheet of pictures) on the GPU
(srlz.ops.decoded_to_bgr / decoded_to_sheet, csrc/latent.hip) and crosses to the host once per image (once per sheet).

Departures from the reference:
  * the window backend is injectable (main(gui=...)): an object with cv2's namedWindow, resizeWindow, createTrackbar, getTrackbarPos,
    getWindowProperty, waitKey, imshow, destroyAllWindows, imread and WINDOW_NORMAL.  The default is cv2, imported when the loop
    starts, never at module import; without cv2 and without --sheet-dir main() says so and exits with status 1;
  * --sheet-dir DIR writes, per figure, DIR/<figure name, spaces as underscores>.png — row = dimension of the block, column =
    slider position (--steps positions from 0 to 100, the other sliders at 50) — and DIR/traversal.json; no window, no cv2;
  * --no-cuda, or a machine without a GPU, raises: this build has no CPU path;
  * a dense auto-encoder (--model-type mlp | linear) shows pictures: its flat decoded vector is viewed as [C, W, H], as the model's
    own forward views it.  The reference hands the flat vector to deNormalize and dies on its assertion ("Color channel must be at
    the end of the tensor (150528,)"), so it has no behaviour to keep there;
  * the running statistics the loaded model came with are put back after every decode, so what is shown never depends on what was
    shown before (in the reference they drift unobserved: training-mode BatchNorm does not read them).
"""
from __future__ import print_function, division, absolute_import

import argparse
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch as th

from models.learner import SRL4robotics, MAX_BATCH_SIZE_GPU, _requireGpu
from preprocessing.preprocess import getNChannels, IMAGE_WIDTH, IMAGE_HEIGHT
from srlz import ops
from utils import detachToNumpy, printRed

VALID_MODELS = ["forward", "inverse", "reward", "priors", "episode-prior", "reward-prior", "triplet",
                "autoencoder", "vae", "dae", "random"]
AUTOENCODERS = ['autoencoder', 'vae', 'dae']
BATCHNORM_MODES = ("reference", "running")
N_NEIGHBORS = 5  # KNeighborsClassifier's default
SHEET_GAP = 2    # pixels between the tiles of a sheet and around it
SHEET_FILL = 255


def _defaultGui():
    import cv2
    return cv2


def getImage(srl_model, state, device):
    """
    Gets an image by using the decoder of a SRL model
    (when available)

    :param srl_model: (Pytorch model)
    :param state: ([float]) the state vector from latent space
    :param device: (pytorch device)
    :return: ([float]) [H, W, 3] BGR float32 in [0, 1]
    """
    with th.no_grad():
        state = th.from_numpy(np.array(state).reshape(1, -1)).float()
        state = state.to(device)
        net_out = _decode(srl_model, state)
        _assertThreeChannels(net_out)
        img = detachToNumpy(ops.decoded_to_bgr(net_out))[0]
    return img


def _decode(srl_model, states):
    """srl_model.decode(states) as images [N, C, W, H].  The dense auto-encoders (--model-type mlp | linear) decode into the flat
    [N, C * W * H] vector, which BaseModelAutoEncoder.forward views as the input's shape: the same view here."""
    net_out = srl_model.decode(states)
    if net_out.dim() == 2:
        net_out = net_out.view(net_out.size(0), getNChannels(), IMAGE_WIDTH, IMAGE_HEIGHT)
    return net_out


def _assertThreeChannels(net_out):
    """deNormalize's assertion on the transposed image (reference preprocessing/utils.py:49), with its text."""
    shape = (int(net_out.shape[3]), int(net_out.shape[2]), int(net_out.shape[1]))
    assert shape[-1] == 3, "Color channel must be at the end of the tensor {}".format(shape)


def createFigureAndSlider(name, state_dim, gui=None):
    """
    Creating a window for the latent space visualization, an another for the slider to control it
    :param name: name of model (str)
    :param state_dim: (int)
    :param gui: the window backend (default: cv2)
    """
    gui = gui if gui is not None else _defaultGui()
    gui.namedWindow(name, gui.WINDOW_NORMAL)
    gui.resizeWindow(name, 500, 500)
    gui.namedWindow('slider for ' + name)
    # add a slider for each component of the latent space
    for i in range(state_dim):
        # the sliders MUST be between 0 and max, so we placed max at 100, and start at 50
        gui.createTrackbar(str(i), 'slider for ' + name, 50, 100, (lambda a: None))


def lossBlocks(exp_config):
    """The figures of an experiment (reference :72-86): loss name -> (start, end), the block's columns of the state.
    One block per sized entry of an OrderedDict `split-dimensions` (a lone entry counts whatever its size, shared -1 entries get
    none); otherwise ONE block, losses[0] over the whole state.  The reference's two prints stay."""
    losses = exp_config['losses']
    state_dim = exp_config['state-dim']
    split_dimensions = exp_config.get('split-dimensions')
    loss_dims = OrderedDict()
    if split_dimensions is not None and isinstance(split_dimensions, OrderedDict):
        for loss_name, loss_dim in split_dimensions.items():
            print(loss_name, loss_dim)
            if loss_dim > 0 or len(split_dimensions) == 1:
                loss_dims[loss_name] = loss_dim
    if len(loss_dims) == 0:
        print(losses)
        loss_dims = {losses[0]: state_dim}
    blocks, start_idx = OrderedDict(), 0
    for loss_name, loss_dim in loss_dims.items():
        blocks[loss_name] = (start_idx, start_idx + loss_dim)
        start_idx += loss_dim
    return blocks


def loadStates(log_dir):
    """image_to_state.json of a log folder (reference :88-91) -> (X float64 [N, S], y: the image paths in the file's order)."""
    with open(log_dir + 'image_to_state.json') as f:
        data = json.load(f)
    X = np.array(list(data.values())).astype(float)
    y = list(data.keys())
    return X, y


def figureName(loss_name):
    return "Decoder for {}".format(loss_name) if loss_name in AUTOENCODERS else "KNN on " + str(loss_name)


def blockBounds(X, start, end):
    """(bound_min, bound_max) of a block: the column extrema of the stored states (reference :110-111)."""
    return np.min(X[:, start:end], axis=0), np.max(X[:, start:end], axis=0)


def sliderState(positions, bound_min, bound_max):
    """Slider positions in [0, 100] -> the block's state, rescaled to the bounds of the representation (reference :129)."""
    return (np.array(positions) / 100) * (bound_max - bound_min) + bound_min


def fullState(state_dim, start, end, state):
    """The block's state with all the other dimensions masked with zeros (reference :132-133)."""
    full_state = np.zeros(state_dim)
    full_state[start:end] = state
    return full_state


def knnImageIndex(X_block, state):
    """KNeighborsClassifier().fit(X_block, np.arange(N)).predict([state])[0] (reference :105-107, :138).  Every label occurs once, so
    the vote among the 5 nearest rows is a 5-way tie that sklearn gives to the smallest label: the result is the smallest INDEX
    among the five nearest rows, not the nearest row.  The search is srlz.ops.knn (exact fp64, ties to the lower index)."""
    X_block = np.asarray(X_block, dtype=np.float64)
    n = X_block.shape[0]
    if n < N_NEIGHBORS:
        raise ValueError("Expected n_neighbors <= n_samples_fit, but n_neighbors = {}, n_samples_fit = {}, n_samples = 1".format(
            N_NEIGHBORS, n))
    idx, _ = ops.knn(X_block, N_NEIGHBORS, queries=np.asarray(state, dtype=np.float64).reshape(1, -1))
    return int(idx[0].min())


def knnImagePath(y, index):
    """The frame of row `index`: a trailing .jpg is removed if present, then data/<path>.jpg (reference :138-141)."""
    return "data/" + y[index].split('.jpg')[0] + ".jpg"


class _KeepBuffers(object):
    """Puts a module's buffers (the BatchNorm running statistics) and its mode back on exit."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.training = self.model.training
        self.saved = [(b, b.detach().clone()) for b in self.model.buffers()]
        return self

    def __exit__(self, *exc):
        with th.no_grad():
            for b, saved in self.saved:
                b.copy_(saved)
        self.model.train(self.training)
        return False


def decodeStates(model, states, batchnorm="reference"):
    """model.decode of several states -> the decoded [N, 3, W, H] device tensor (C channels for a multi-view model).
    :param model: the auto-encoder (what getImage receives)
    :param states: [N, S] array; cast to float32 as getImage casts one state
    :param batchnorm: "reference": every state is decoded ALONE with the model in training mode — one tick of the reference, whose
        BatchNorm layers see the statistics of that one image; "running": eval mode on the running statistics, one batched call per
        at most MAX_BATCH_SIZE_GPU states.  Either way the model's buffers and mode are as before afterwards.
        (The dense auto-encoders have no BatchNorm: both routes give the same images.)"""
    if batchnorm not in BATCHNORM_MODES:
        raise ValueError("batchnorm must be one of {} (got {!r})".format(BATCHNORM_MODES, batchnorm))
    device = next(model.parameters()).device
    states = th.from_numpy(np.array(states, dtype=np.float64).reshape(len(states), -1)).float().to(device)
    per = 1 if batchnorm == "reference" else MAX_BATCH_SIZE_GPU
    with th.no_grad(), _KeepBuffers(model):
        model.train(batchnorm == "reference")
        out = [_decode(model, states[i:i + per].contiguous()) for i in range(0, len(states), per)]
    return out[0] if len(out) == 1 else th.cat(out, dim=0)


def traversalStates(state_dim, start, end, bound_min, bound_max, positions):
    """The states of a block's sheet: for every dimension i of the block and every position p, slider i at p and the others at 50.
    :return: ([dim * len(positions), state_dim] full states, the same number of block states), row-major (dimension, position)"""
    dim = end - start
    full, block = [], []
    for i in range(dim):
        for p in positions:
            sliders = [50] * dim
            sliders[i] = int(p)
            state = sliderState(sliders, bound_min, bound_max)
            block.append(state)
            full.append(fullState(state_dim, start, end, state))
    return np.array(full).reshape(dim * len(positions), state_dim), np.array(block).reshape(dim * len(positions), dim)


def hostSheet(images, cols, gap=SHEET_GAP, fill=SHEET_FILL):
    """uint8 [h, w, 3] images of one size -> the sheet decoded_to_sheet lays out, assembled on the host."""
    h, w = images[0].shape[:2]
    for im in images:
        if im.shape != (h, w, 3):
            raise ValueError("the frames of a sheet must all be {} x {} x 3 (got {})".format(h, w, im.shape))
    sh, sw = ops.sheet_size(len(images), w, h, cols, gap)
    sheet = np.full((sh, sw, 3), fill, dtype=np.uint8)
    for i, im in enumerate(images):
        top, left = gap + (i // cols) * (h + gap), gap + (i % cols) * (w + gap)
        sheet[top:top + h, left:left + w] = im
    return sheet


def writeSheets(model, exp_config, X, y, blocks, sheet_dir, steps, cols, batchnorm):
    """The headless mode: one PNG per figure and traversal.json."""
    from PIL import Image
    if steps < 1:
        raise ValueError("--steps must be at least 1 (got {})".format(steps))
    os.makedirs(sheet_dir, exist_ok=True)
    state_dim = exp_config['state-dim']
    positions = np.round(np.linspace(0, 100, steps)).astype(int)
    cols = cols if cols else steps
    record = []
    for loss_name, (start, end) in blocks.items():
        name = figureName(loss_name)
        bound_min, bound_max = blockBounds(X, start, end)
        full, block = traversalStates(state_dim, start, end, bound_min, bound_max, positions)
        entry = OrderedDict([("name", name), ("start", start), ("end", end), ("positions", [int(p) for p in positions]),
                             ("bound_min", [float(v) for v in bound_min]), ("bound_max", [float(v) for v in bound_max])])
        if loss_name in AUTOENCODERS:
            dec = decodeStates(model.model, full, batchnorm)
            _assertThreeChannels(dec)
            # (one device-to-host copy per sheet)
            sheet = ops.decoded_to_sheet(dec, cols, gap=SHEET_GAP, fill=SHEET_FILL, rgb=True).cpu().numpy()
        else:
            X_block = X[:, start:end]
            paths = [knnImagePath(y, knnImageIndex(X_block, state)) for state in block]
            entry["images"] = paths
            frames = {}
            for p in paths:
                if p not in frames:
                    with Image.open(p) as f:
                        frames[p] = np.asarray(f.convert("RGB"))
            sheet = hostSheet([frames[p] for p in paths], cols)
        Image.fromarray(sheet).save(os.path.join(sheet_dir, name.replace(" ", "_") + ".png"))
        record.append(entry)
    with open(os.path.join(sheet_dir, "traversal.json"), "w") as f:
        json.dump(record, f, indent=2)
    return record


def runWindows(model, exp_config, X, y, blocks, gui, device, batchnorm):
    """The reference's loop (:93-150) on the window backend `gui`."""
    state_dim = exp_config['state-dim']
    bound_max, bound_min, fig_names = {}, {}, {}
    for loss_name, (start, end) in blocks.items():
        bound_min[loss_name], bound_max[loss_name] = blockBounds(X, start, end)
        fig_names[loss_name] = figureName(loss_name)
        createFigureAndSlider(fig_names[loss_name], end - start, gui)
    # the reference leaves the loaded model as nn.Module makes it: in training mode
    model.train(batchnorm == "reference")

    should_exit = False
    while not should_exit:
        # stop if escape is pressed
        k = gui.waitKey(1) & 0xFF
        if k == 27:
            break

        for loss_name, (start, end) in blocks.items():
            state = []
            for i in range(end - start):
                state.append(gui.getTrackbarPos(str(i), 'slider for ' + fig_names[loss_name]))
            # Rescale the values to fit the bounds of the representation
            state = sliderState(state, bound_min[loss_name], bound_max[loss_name])
            # Mask all the irrelevant dimensions with zeros
            full_state = fullState(state_dim, start, end, state)

            if loss_name in AUTOENCODERS:
                with _KeepBuffers(model):
                    img = getImage(model.model, full_state, device)
            else:
                img = gui.imread(knnImagePath(y, knnImageIndex(X[:, start:end], state)))

            # stop if user closed a window
            if (gui.getWindowProperty(fig_names[loss_name], 0) < 0) or \
                    (gui.getWindowProperty('slider for ' + fig_names[loss_name], 0) < 0):
                should_exit = True
                break
            gui.imshow(fig_names[loss_name], img)

    # gracefully close
    gui.destroyAllWindows()


def build_parser():
    parser = argparse.ArgumentParser(description="latent space enjoy")
    parser.add_argument('--log-dir', default='', type=str, help='directory to load model')
    parser.add_argument('--no-cuda', default=False, action="store_true")
    parser.add_argument('--batchnorm', default="reference", choices=BATCHNORM_MODES,
                        help="reference: decode every state alone on its own batch statistics, as the reference does; "
                             "running: eval mode on the running statistics")
    parser.add_argument('--sheet-dir', default=None, type=str, help='write traversal sheets (PNG) there instead of opening windows')
    parser.add_argument('--steps', default=11, type=int, help='slider positions per dimension of a sheet (default: 11)')
    parser.add_argument('--cols', default=None, type=int, help='columns of a sheet (default: --steps, so row = dimension)')
    return parser


def main(argv=None, gui=None):
    args = build_parser().parse_args(argv)
    if args.sheet_dir is None and gui is None:
        try:
            gui = _defaultGui()
        except ImportError:
            printRed("enjoy_latent needs cv2 for its windows and cv2 is not installed: use --sheet-dir DIR to write the "
                     "traversal sheets as PNG files instead")
            sys.exit(1)
    use_cuda = not args.no_cuda
    _requireGpu(use_cuda)
    device = th.device("cuda", th.cuda.current_device())

    srl_model, exp_config = SRL4robotics.loadSavedModel(args.log_dir, VALID_MODELS, cuda=use_cuda)
    # Retrieve the pytorch model
    srl_model = srl_model.model
    blocks = lossBlocks(exp_config)
    # Load all the states and images
    X, y = loadStates(args.log_dir)

    if args.sheet_dir is not None:
        writeSheets(srl_model, exp_config, X, y, blocks, args.sheet_dir, args.steps, args.cols, args.batchnorm)
    else:
        runWindows(srl_model, exp_config, X, y, blocks, gui, device, args.batchnorm)


if __name__ == '__main__':
    main()
