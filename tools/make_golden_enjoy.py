#!/usr/bin/env python
"""Generate tests/golden/enjoy_kats.npz and tests/golden/enjoy_spread.json by running the UNMODIFIED reference
evaluation/enjoy_latent.py on seeded models.  The reference is executed from its own file, never copied; cv2, absent here, is a
stand-in module (tests/enjoy_util.py::ScriptedGui) that scripts the trackbar positions tick by tick, records every imshow image and
every imread path and answers waitKey with 27 after the last scripted tick; the other absent modules are stubbed as
tools/make_golden.py stubs them.  Runs where the reference lives only.

Log folders are built with the reference's own SRL4robotics on the CPU (seeded initialisation, no training); the cases, their states
and their slider scripts are the descriptors of tests/enjoy_util.py, which the tests regenerate them from.

Recorded per shown image: the loop's own state and full state, the fp64 sum and sum of squares of the image, its stride-4 subsample
and, for nearest-frame ticks, the chosen path; per case the digest of the model's state_dict.

For nearest-frame ticks the tool asserts that the 6 smallest fp64 distances of every query are more than 1e-9 apart (relative), so
no fixture hangs on a tie, and that at least one query's nearest row is NOT the smallest index of its five.

enjoy_spread.json: every decoded fixture state once more with the reference model converted to float64 (same training-mode decode of
one state, deNormalize and clip in float64); per case the largest absolute difference to the float32 image.

    python tools/make_golden_enjoy.py            # each case in a fresh interpreter
"""
from __future__ import print_function
import json
import os
import runpy
import subprocess
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REPO, "tests"))

import enjoy_util as eu  # noqa: E402
import knn_util as ku  # noqa: E402

MIN_GAP = 1e-9
MAX_BYTES = 605060  # the largest fixture of tests/golden before this one (trace10_ae_b32.npz)


def _stub_modules(gui):
    tv = types.ModuleType("torchvision")
    tvm = types.ModuleType("torchvision.models")
    tvm.resnet18 = lambda *a, **k: None
    tv.models = tvm
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.models"] = tvm
    tc = types.ModuleType("termcolor")
    tc.colored = lambda s, *a, **k: s
    sys.modules["termcolor"] = tc
    sb = types.ModuleType("seaborn")
    sb.set = lambda *a, **k: None
    sys.modules["seaborn"] = sb
    sys.modules["cv2"] = gui.as_module(types.ModuleType("cv2"))
    import matplotlib
    matplotlib.use("Agg")


def float64_image(th, model, full_state):
    """getImage with the model in float64: the reference's arithmetic, every step in double."""
    with th.no_grad():
        out = model.decode(th.from_numpy(np.array(full_state).reshape(1, -1)).float().double())
    x = out.numpy().reshape(1, 3, 224, 224)[0].T.copy()
    x *= np.array([0.229, 0.224, 0.225])
    x += np.array([0.485, 0.456, 0.406])
    return np.clip(x, 0, 1)[:, :, ::-1]


def viewed_ticks(th, case, X, twin, gui):
    """The ticks of a dense auto-encoder, which the reference's script cannot show: its loop's arithmetic (:129-133) and its getImage
    (:31-39) on the reference's model and deNormalize, with ONE step added — the flat decoded vector viewed as [1, 3, 224, 224], as
    BaseModelAutoEncoder.forward views it.  Appends to gui.shown what the script's imshow would have recorded."""
    from preprocessing.utils import deNormalize  # the reference's
    model32 = twin.model.float()
    for t, tick in enumerate(gui.script):
        for loss, start, end in eu.case_blocks(case):
            name = eu.figure_name(loss)
            bound_min, bound_max = np.min(X[:, start:end], axis=0), np.max(X[:, start:end], axis=0)
            state = (np.array(tick["slider for " + name]) / 100) * (bound_max - bound_min) + bound_min
            full_state = np.zeros(case["state_dim"])
            full_state[start:end] = state
            with th.no_grad():
                net_out = model32.decode(th.from_numpy(np.array(full_state).reshape(1, -1)).float()).view(1, 3, 224, 224)
                img = net_out.numpy()[0].T
            img = deNormalize(img, mode="image_net")[:, :, ::-1]
            gui.shown.append(dict(tick=t, name=name, img=np.array(img, copy=True), state=state, full_state=full_state))
    twin.double()


def run_case(case):
    gui = eu.ScriptedGui(eu.case_script(case))
    _stub_modules(gui)
    sys.path.insert(0, REF)
    import torch as th
    th.set_num_threads(1)  # single-threaded: deterministic summation order
    import models.learner as RL  # the reference's
    out = {}
    cwd, argv = os.getcwd(), list(sys.argv)
    with tempfile.TemporaryDirectory() as root:
        log = os.path.join(root, "logs", case["name"]) + "/"
        srl = RL.SRL4robotics(case["state_dim"], model_type=case["model_type"], seed=case["seed"], cuda=False, losses=case["losses"],
                              n_actions=eu.N_ACTIONS, split_dimensions=eu.split_dimensions(case), log_folder=log)
        sd = srl.model.state_dict()
        eu.write_log_folder(log, case, sd, th.save)
        out["sd_names"] = np.array(list(sd.keys()))
        out["sd_sums"], out["sd_abss"] = eu.state_dict_digest(sd)
        os.chdir(root)
        try:
            sys.argv = ["enjoy_latent.py", "--log-dir", log, "--no-cuda"]
            runpy.run_path(os.path.join(REF, "evaluation", "enjoy_latent.py"), run_name="__main__")
            assert case["model_type"] == "custom_cnn", "the reference is expected to fail on a dense auto-encoder"
            assert gui.destroyed and gui.tick == len(gui.script)
        except AssertionError as e:
            # a dense auto-encoder decodes into a flat vector, which the reference hands to deNormalize: it dies on the first tick
            if case["model_type"] == "custom_cnn":
                raise
            out["reference_error"] = np.array(str(e))
            assert str(e) == "Color channel must be at the end of the tensor (150528,)" and not gui.shown, str(e)
        finally:
            os.chdir(cwd)
            sys.argv = argv
        # the float64 twin of the loaded model, in the mode the script left it in (training: it never calls eval())
        twin, _ = RL.SRL4robotics.loadSavedModel(log, ["autoencoder", "vae", "dae", "inverse"], cuda=False)
        twin = twin.model.double()
        assert twin.training
    X = np.array([[float(str(v)) for v in row] for row in eu.case_states(case)])
    blocks = {eu.figure_name(loss): (loss, start, end) for loss, start, end in eu.case_blocks(case)}
    if "reference_error" in out:
        viewed_ticks(th, case, X, twin, gui)
    out["windows"] = np.array(gui.windows)
    out["n_shown"] = np.array(len(gui.shown))
    spread, off_nearest = 0.0, 0
    reads = list(gui.reads)
    for i, rec in enumerate(gui.shown):
        loss, start, end = blocks[rec["name"]]
        key = "shown%02d/" % i
        out[key + "tick"] = np.array(rec["tick"])
        out[key + "name"] = np.array(rec["name"])
        out[key + "state"] = np.asarray(rec["state"], dtype=np.float64)
        out[key + "full_state"] = np.asarray(rec["full_state"], dtype=np.float64)
        if loss in eu.AUTOENCODERS:
            img = rec["img"]
            assert img.dtype == np.float32 and img.shape == (224, 224, 3), (img.dtype, img.shape)
            out[key + "sum"] = np.float64(img.astype(np.float64).sum())
            out[key + "sumsq"] = np.float64((img.astype(np.float64) ** 2).sum())
            out[key + "sub"] = np.ascontiguousarray(img[::eu.SUBSAMPLE, ::eu.SUBSAMPLE])
            spread = max(spread, float(np.abs(float64_image(th, twin.model, rec["full_state"]) - img.astype(np.float64)).max()))
        else:
            tick, path = reads.pop(0)
            assert tick == rec["tick"] and path == "data/" + rec["img_path"] + ".jpg", (tick, path, rec)
            out[key + "path"] = np.array(path)
            idx, d2 = ku.brute_knn(X[:, start:end], rec["state"][None], 6)
            gap = float(ku.relative_gaps(d2).min())
            assert gap > MIN_GAP, (case["name"], i, gap)
            chosen = int(idx[0, :5].min())
            assert eu.case_paths(case)[chosen].split(".jpg")[0] == rec["img_path"], (case["name"], i, chosen, rec["img_path"])
            off_nearest += int(idx[0, 0] != chosen)
            out[key + "nearest"] = np.array(int(idx[0, 0]))
            out[key + "min_gap"] = np.float64(gap)
    assert not reads
    if any(loss not in eu.AUTOENCODERS for loss, _, _ in blocks.values()):
        assert off_nearest >= 1, "no query of %s has a nearest row that is not the smallest index of its five" % case["name"]
    return out, spread


def child(name, path):
    out, spread = run_case(eu.case_by_name(name))
    out["spread"] = np.float64(spread)
    np.savez(path, **out)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3])
    merged, spreads = {}, {}
    for case in eu.CASES:
        tmp = tempfile.mktemp(suffix=".npz")
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", case["name"], tmp], timeout=1500)
        with np.load(tmp, allow_pickle=False) as z:
            for k in z.files:
                if k == "spread":
                    spreads[case["name"]] = float(z[k])
                else:
                    merged["%s/%s" % (case["name"], k)] = z[k]
        os.remove(tmp)
        print("%-18s %d shown images, float32-to-float64 spread %.3e" % (case["name"], int(merged[case["name"] + "/n_shown"]),
                                                                         spreads[case["name"]]))
    merged["cases"] = np.array(json.dumps(eu.CASES))
    import sklearn
    merged["sklearn_version"] = np.array(sklearn.__version__)
    np.savez_compressed(eu.GOLDEN, **merged)
    size = os.path.getsize(eu.GOLDEN)
    print("wrote %s (%d bytes; the largest fixture before it has %d)" % (eu.GOLDEN, size, MAX_BYTES))
    assert size <= MAX_BYTES, "enjoy_kats.npz would be the largest fixture of tests/golden: store fewer ticks"
    with open(eu.SPREAD, "w") as f:
        json.dump(spreads, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s" % eu.SPREAD)


if __name__ == "__main__":
    main()
