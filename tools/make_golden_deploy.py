#!/usr/bin/env python
"""Generate tests/golden/deploy_kats.npz and tests/golden/deploy_spread.json by running the UNMODIFIED reference model classes on the
CPU.  The reference is imported from its own files, never copied; the modules it imports that are absent here are stubbed as
tools/make_golden.py stubs them.  Runs where the reference lives only.

Per model of tests/deploy_util.py::CASES (custom_cnn + inverse S = 3, autoencoder S = 8, vae S = 8, split autoencoder:1:4
inverse:1:4, multi-view autoencoder C = 6):
  * seeded construction of the reference's SRLModules / SRLModulesSplit (deploy_util.build_case), BatchNorm gamma, beta and running
    statistics from the closed form deploy_util.bn_formula; the parameters' checksums are stored, not the weights;
  * three 224 x 224 frames from the integer formula deploy_util.frames_nhwc (no frame is stored), through the reference's
    preprocessInput per camera (preprocessing/utils.py:6-35) and the loader's transpose (preprocessing/data_loader.py:255);
  * eval-mode getStates in fp32 and, with the model converted to float64, in fp64.
deploy_kats.npz holds the expected states (both precisions) and the checksums; deploy_spread.json the reference's own fp32-to-fp64
spread per model, max |s32 - s64| / max |s64| — the tests' bound is max(1e-4, 10 x that spread) of the states' scale.

    python tools/make_golden_deploy.py
"""
from __future__ import print_function
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SRLZ_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "tests"))
GOLDEN = os.path.join(REPO, "tests", "golden", "deploy_kats.npz")
SPREAD = os.path.join(REPO, "tests", "golden", "deploy_spread.json")
MAX_BYTES = 605060  # the largest fixture of tests/golden (trace10_ae_b32.npz): these stay far below it


def _stub_modules():
    tv = types.ModuleType("torchvision")
    tvm = types.ModuleType("torchvision.models")
    tvm.resnet18 = lambda *a, **k: None
    tv.models = tvm
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.models", tvm)
    tc = types.ModuleType("termcolor")
    tc.colored = lambda s, *a, **k: s
    sys.modules.setdefault("termcolor", tc)
    sb = types.ModuleType("seaborn")
    sb.set = lambda *a, **k: None
    sys.modules.setdefault("seaborn", sb)
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))  # (imported by the loader, which this tool never runs)
    import matplotlib
    matplotlib.use("Agg")


def reference_input(pre_utils, frames):
    """uint8 [N,H,W,C] -> the reference's observation tensor [N,C,W,H] (numpy fp32): preprocessInput per camera, dstack, transpose."""
    out = []
    for fr in frames:
        cams = [pre_utils.preprocessInput(fr[..., g:g + 3].astype(np.float32), mode="image_net") for g in range(0, fr.shape[-1], 3)]
        im = np.dstack(cams)
        out.append(im.reshape((1,) + im.shape).transpose(0, 3, 2, 1))
    return np.ascontiguousarray(np.concatenate(out, 0))


def main():
    _stub_modules()
    sys.path.insert(0, REF)
    import torch as th
    th.set_num_threads(1)  # single-threaded: deterministic summation order
    import deploy_util as du
    import models.modules as ref_modules  # the reference's
    import preprocessing.preprocess as ref_pre
    import preprocessing.utils as ref_utils
    assert os.path.abspath(ref_modules.__file__).startswith(os.path.abspath(REF)), ref_modules.__file__
    merged, spreads = {}, {}
    for name in du.CASES:
        model = du.build_case(name, ref_modules, ref_pre)
        model.eval()
        names, sums, abss = du.checksums(model.state_dict())
        x = th.from_numpy(reference_input(ref_utils, du.case_frames(name)))
        with th.no_grad():
            s32 = model.getStates(x).numpy().astype(np.float32)
            s64 = model.double().getStates(x.double()).numpy().astype(np.float64)
        assert s32.shape == (du.N_FRAMES, du.CASES[name]["state_dim"]) and np.isfinite(s64).all()
        spreads[name] = float(np.abs(s32.astype(np.float64) - s64).max() / np.abs(s64).max())
        merged[name + "/names"], merged[name + "/sums"], merged[name + "/abss"] = np.array(names), sums, abss
        merged[name + "/states32"], merged[name + "/states64"] = s32, s64
        print("%-18s states scale %.4f, fp32-to-fp64 spread %.3e" % (name, np.abs(s64).max(), spreads[name]))
    np.savez_compressed(GOLDEN, **merged)
    with open(SPREAD, "w") as f:
        json.dump(spreads, f, indent=1, sort_keys=True)
        f.write("\n")
    for p in (GOLDEN, SPREAD):
        size = os.path.getsize(p)
        print("wrote %s (%d bytes; the largest fixture has %d)" % (p, size, MAX_BYTES))
        assert size < MAX_BYTES // 10


if __name__ == "__main__":
    main()
