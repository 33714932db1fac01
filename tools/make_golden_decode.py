#!/usr/bin/env python
"""Generate tests/golden/decode_kats.npz and tests/golden/decode_spread.json by running the UNMODIFIED reference model classes on the
CPU.  The reference is imported from its own files, never copied; the modules it imports that are absent here are stubbed as
tools/make_golden_deploy.py stubs them.  Runs where the reference lives only.

Per model of tests/decode_util.py::CASES (autoencoder S = 8, vae S = 8, split autoencoder:1:4 inverse:1:4, multi-view autoencoder
C = 6):
  * seeded construction of the reference's SRLModules / SRLModulesSplit (decode_util.build_case), every BatchNorm's gamma, beta and
    running statistics from the closed form deploy_util.bn_formula (decoder: layers 3..6); the parameters' checksums are stored, not
    the weights;
  * three states from the integer formula decode_util.states (no state is stored);
  * eval-mode decode of the network behind the wrapper (what evaluation/enjoy_latent.py:21-39 calls) in fp32 and, with the model
    converted to float64, in fp64.
decode_kats.npz holds, per model, the fp64 decode on the pixel lattice decode_util.LATTICE (the four outermost rows and columns at
every edge included), the fp64 sum and sum of squares of every full (image, channel) plane, and the checksums; decode_spread.json the
reference's own fp32-to-fp64 spread per model, max |d32 - d64| / max |d64| — the tests' bound is max(1e-4, 10 x that spread).

    python tools/make_golden_decode.py
"""
from __future__ import print_function
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
GOLDEN = os.path.join(REPO, "tests", "golden", "decode_kats.npz")
SPREAD = os.path.join(REPO, "tests", "golden", "decode_spread.json")
MAX_BYTES = 605060  # the largest fixture of tests/golden (trace10_ae_b32.npz)


def main():
    from make_golden_deploy import _stub_modules, REF  # (the reference checkout: SRLZ_REFERENCE)
    _stub_modules()
    sys.path.insert(0, REF)
    import torch as th
    th.set_num_threads(1)  # single-threaded: deterministic summation order
    import deploy_util as du
    import decode_util as dd
    import models.modules as ref_modules  # the reference's
    import preprocessing.preprocess as ref_pre
    assert os.path.abspath(ref_modules.__file__).startswith(os.path.abspath(REF)), ref_modules.__file__
    merged, spreads = {}, {}
    for name in dd.CASES:
        model = dd.build_case(name, ref_modules, ref_pre)
        model.eval()
        names, sums, abss = du.checksums(model.state_dict())
        z = th.from_numpy(dd.case_states(name))
        with th.no_grad():
            d32 = model.model.decode(z).numpy().astype(np.float32)
            d64 = model.double().model.decode(z.double()).numpy().astype(np.float64)
        c = du.CASES[name]["channels"]
        assert d32.shape == (dd.N_STATES, c, 224, 224) and np.isfinite(d64).all()
        spreads[name] = float(np.abs(d32.astype(np.float64) - d64).max() / np.abs(d64).max())
        v = dd.denormalize64(d64)
        inside = float(((v > 0.02) & (v < 0.98)).mean())
        assert inside >= 0.9, (name, inside)
        by = dd.bytes_expr(d32)
        s1, s2 = dd.plane_sums(d64)
        merged[name + "/names"], merged[name + "/sums"], merged[name + "/abss"] = np.array(names), sums, abss
        merged[name + "/lattice64"], merged[name + "/plane_sum"], merged[name + "/plane_sumsq"] = dd.lattice(d64), s1, s2
        print("%-18s decode scale %.4f, fp32-to-fp64 spread %.3e, denormalised in [%.3f, %.3f] (%.1f %% inside (0.02, 0.98)), "
              "byte std %.1f" % (name, np.abs(d64).max(), spreads[name], v.min(), v.max(), 100 * inside, by.astype(np.float64).std()))
    np.savez_compressed(GOLDEN, **merged)
    with open(SPREAD, "w") as f:
        json.dump(spreads, f, indent=1, sort_keys=True)
        f.write("\n")
    for p in (GOLDEN, SPREAD):
        size = os.path.getsize(p)
        print("wrote %s (%d bytes; the largest fixture has %d)" % (p, size, MAX_BYTES))
        assert size < MAX_BYTES


if __name__ == "__main__":
    main()
