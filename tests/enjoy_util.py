"""Shared by the enjoy_latent tests and tools/make_golden_enjoy.py: the fixture cases of tests/golden/enjoy_kats.npz (the fixture
records results only; log folders, states and slider scripts are regenerated here from the descriptors), the scripted window backend
that stands in for cv2, and the numpy restatements of the image kernels of csrc/latent.hip."""
import json
import os
import sys
from collections import OrderedDict

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "enjoy_kats.npz")
SPREAD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "enjoy_spread.json")

N_ACTIONS = 6
N_ROWS = 40       # rows of a fixture's image_to_state.json
SUBSAMPLE = 4     # stride of the stored part of a shown image

# name, constructor arguments, seed of the constructor and of the states.  split: the --losses name:weight:dim form as the
# OrderedDict train.py makes of it.
CASES = [
    dict(name="cnn_ae", model_type="custom_cnn", losses=["autoencoder"], state_dim=4, split=None, seed=11),
    dict(name="cnn_vae", model_type="custom_cnn", losses=["vae"], state_dim=3, split=None, seed=12),
    dict(name="cnn_inverse", model_type="custom_cnn", losses=["inverse"], state_dim=3, split=None, seed=13),
    dict(name="split_ae_inverse", model_type="custom_cnn", losses=["autoencoder", "inverse"], state_dim=4,
         split=[["autoencoder", 2], ["inverse", 2]], seed=14),
    dict(name="mlp_ae", model_type="mlp", losses=["autoencoder"], state_dim=3, split=None, seed=15),
]
AUTOENCODERS = ("autoencoder", "vae", "dae")


def case_by_name(name):
    return [c for c in CASES if c["name"] == name][0]


def split_dimensions(case):
    return OrderedDict((k, v) for k, v in case["split"]) if case["split"] else -1


def case_states(case):
    """The learned states of a fixture: float32 values, as learn() stores them."""
    return (np.random.RandomState(100 + case["seed"]).randn(N_ROWS, case["state_dim"]) * 1.5).astype(np.float32)


def case_paths(case):
    """Image paths of the rows; every third carries the trailing .jpg the script strips."""
    return ["enjoy_kats/record_%03d/frame%06d%s" % (i // 20, i % 20, ".jpg" if i % 3 == 0 else "") for i in range(N_ROWS)]


def case_blocks(case):
    """[(loss name, start, end)]: the figures the reference opens for the case."""
    if case["split"]:
        out, start = [], 0
        for k, v in case["split"]:
            if v > 0 or len(case["split"]) == 1:
                out.append((k, start, start + v))
                start += v
        return out
    return [(case["losses"][0], 0, case["state_dim"])]


def figure_name(loss):
    return "Decoder for %s" % loss if loss in AUTOENCODERS else "KNN on %s" % loss


def case_script(case):
    """The scripted ticks: per tick {slider window: [positions]}.  All sliders at 50, at 0 and at 100, then seeded positions."""
    rs = np.random.RandomState(200 + case["seed"])
    n_ticks = 5 if case["name"] == "cnn_inverse" else 4
    ticks = []
    for t in range(n_ticks):
        tick = OrderedDict()
        for loss, start, end in case_blocks(case):
            dim = end - start
            pos = [50] * dim if t == 0 else [0] * dim if t == 1 else [100] * dim if t == 2 else [int(p) for p in rs.randint(0, 101, dim)]
            tick["slider for " + figure_name(loss)] = pos
        ticks.append(tick)
    return ticks


def exp_config(case):
    cfg = OrderedDict([("state-dim", case["state_dim"]), ("losses", case["losses"]), ("n_actions", N_ACTIONS),
                       ("model-type", case["model_type"]), ("multi-view", False), ("inverse-model-type", "linear")])
    if case["split"]:
        cfg["split-dimensions"] = split_dimensions(case)
    return cfg


def write_log_folder(log, case, state_dict, save):
    """exp_config.json, image_to_state.json (values as strings, keys in row order: what saveStates writes, unsorted so that the
    file's order is the rows') and srl_model.pth through `save` (the caller's torch.save) into `log`."""
    os.makedirs(log, exist_ok=True)
    with open(os.path.join(log, "exp_config.json"), "w") as f:
        json.dump(exp_config(case), f)
    table = OrderedDict((p, list(map(str, s))) for p, s in zip(case_paths(case), case_states(case)))
    with open(os.path.join(log, "image_to_state.json"), "w") as f:
        json.dump(table, f)
    save(state_dict, os.path.join(log, "srl_model.pth"))


def state_dict_digest(sd):
    """fp64 sum and sum of absolute values per tensor of a CPU state_dict, in its order."""
    return (np.array([float(v.double().sum()) for v in sd.values()]), np.array([float(v.double().abs().sum()) for v in sd.values()]))


class ScriptedGui(object):
    """The window backend of a scripted session: cv2's calls as enjoy_latent uses them.  Tick t answers getTrackbarPos from
    script[t]; waitKey answers 27 (escape) once the script is used up.  Every imshow and imread is recorded; imshow also looks into
    its caller's frame for the loop's own `state`, `full_state` and (kNN ticks) `img_path`, where the caller has them."""
    WINDOW_NORMAL = 0

    def __init__(self, script):
        self.script = script
        self.tick = -1
        self.windows, self.trackbars, self.shown, self.reads = [], [], [], []
        self.destroyed = False

    def namedWindow(self, name, flags=None):
        self.windows.append(name)

    def resizeWindow(self, name, w, h):
        assert name in self.windows

    def createTrackbar(self, name, window, value, count, on_change):
        assert window in self.windows
        self.trackbars.append((name, window, value, count))

    def getTrackbarPos(self, name, window):
        return self.script[self.tick][window][int(name)]

    def getWindowProperty(self, name, prop):
        return 0.0 if name in self.windows else -1.0

    def waitKey(self, delay):
        self.tick += 1
        return 27 if self.tick >= len(self.script) else -1

    def imread(self, path):
        self.reads.append((self.tick, path))
        return np.zeros((2, 2, 3), dtype=np.uint8)

    def imshow(self, name, img):
        caller = sys._getframe(1).f_locals
        rec = dict(tick=self.tick, name=name, img=np.array(img, copy=True))
        for key in ("state", "full_state", "img_path"):
            if key in caller:
                rec[key] = np.array(caller[key], copy=True) if key != "img_path" else str(caller[key])
        self.shown.append(rec)

    def destroyAllWindows(self):
        self.destroyed = True

    def as_module(self, module):
        """Put the calls on a module object (the cv2 stand-in of tools/make_golden_enjoy.py)."""
        for key in ("WINDOW_NORMAL", "namedWindow", "resizeWindow", "createTrackbar", "getTrackbarPos", "getWindowProperty", "waitKey",
                    "imread", "imshow", "destroyAllWindows"):
            setattr(module, key, getattr(self, key))
        return module


def load_golden():
    """:return: (npz, {case name: largest |float32 - float64| image difference of the reference})"""
    with open(SPREAD) as f:
        spread = json.load(f)
    return np.load(GOLDEN), spread


# ---- numpy restatements of csrc/latent.hip -------------------------------------------------------------------------------------
def numpy_bgr(dec):
    """getImage's numpy expression (reference evaluation/enjoy_latent.py:36-39 with preprocessing/utils.py:54-66) per image of a
    decoded batch [N, 3, W, H] -> float32 [N, H, W, 3]."""
    out = []
    for d in np.asarray(dec, dtype=np.float32):
        x = d.T.copy()
        x[..., 0] *= 0.229
        x[..., 1] *= 0.224
        x[..., 2] *= 0.225
        x[..., 0] += 0.485
        x[..., 1] += 0.456
        x[..., 2] += 0.406
        out.append(np.clip(x, 0, 1)[:, :, ::-1])
    return np.ascontiguousarray(np.stack(out))


def numpy_sheet(bgr, cols, gap, fill, rgb):
    """The sheet of float BGR images [N, H, W, 3]: np.rint(v * np.float32(255)) as bytes, tiled."""
    n, h, w, _ = bgr.shape
    u8 = np.rint(bgr * np.float32(255)).astype(np.uint8)
    if rgb:
        u8 = u8[..., ::-1]
    rows = (n + cols - 1) // cols
    sheet = np.full((rows * h + (rows + 1) * gap, cols * w + (cols + 1) * gap, 3), fill, dtype=np.uint8)
    for i in range(n):
        top, left = gap + (i // cols) * (h + gap), gap + (i % cols) * (w + gap)
        sheet[top:top + h, left:left + w] = u8[i]
    return sheet
