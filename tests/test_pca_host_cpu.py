"""The PCA baseline's host side (no GPU): the reference's command line and batch-size rule, pipeline.pcaCall's argument list, the
host transform of an object rebuilt from recorded fields (what an unpickled pca.pkl does anywhere), the "no CPU path" error of fitting,
the C ABI's new entry points in header, library and binding, and a static audit of the fp64 MFMA kernels' ISA."""
import os
import pickle
import shutil
import sys

import numpy as np
import pytest

import pca_util as pu
from test_cabi_symbols import declared_symbols

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import isa_audit  # noqa: E402

ENTRY_POINTS = ("srlz_pca_workspace", "srlz_pca_transform_workspace", "srlz_pca_stats", "srlz_pca_gram", "srlz_pca_project",
                "srlz_pca_transform")


@pytest.fixture(scope="module")
def kats():
    return pu.load_kats()


def test_parser_has_the_reference_flags_and_defaults():
    from srl_baselines.pca import buildParser, fitBatchSize, getModelName
    a = buildParser().parse_args(["--data-folder", "data/ds/"])
    assert (a.batch_size, a.no_display_plots, a.data_folder, a.training_set_size, a.state_dim) == (16, False, "data/ds/", -1, 3)
    a = buildParser().parse_args(["-bs", "8", "--no-display-plots", "--data-folder", "ds", "--training-set-size", "40", "--state-dim", "5"])
    assert (a.batch_size, a.no_display_plots, a.training_set_size, a.state_dim) == (8, True, 40, 5)
    with pytest.raises(SystemExit):
        buildParser().parse_args([])  # --data-folder is required
    a.method = "pca"
    assert getModelName(a) == "pca_ST_DIM5"
    # batch_size = max(k + 1, bs): sklearn's "Mean of empty slice" guard of the reference
    assert fitBatchSize(3, 16) == 16 and fitBatchSize(200, 16) == 201 and fitBatchSize(15, 16) == 16 and fitBatchSize(16, 16) == 17


def test_pca_call_passes_the_reference_arguments(monkeypatch):
    import subprocess
    import pipeline
    seen = {}

    def fake_call(cmd, **kw):
        seen["cmd"], seen["kw"] = list(cmd), kw
        return 0
    monkeypatch.setattr(subprocess, "call", fake_call)
    pipeline.pcaCall({"data-folder": "ds", "training-set-size": -1, "state-dim": 3, "log-folder": "unused"})
    assert seen["cmd"] == [sys.executable, "-m", "srl_baselines.pca", "--no-display-plots", "--data-folder", "ds",
                           "--training-set-size", "-1", "--state-dim", "3"]
    pkg = os.path.dirname(os.path.abspath(pipeline.__file__))
    assert seen["kw"]["env"]["PYTHONPATH"].split(os.pathsep)[0] == pkg
    from srl_baselines.pca import buildParser
    a = buildParser().parse_args(seen["cmd"][3:])
    assert (a.data_folder, a.training_set_size, a.state_dim, a.no_display_plots) == ("ds", -1, 3, True)
    monkeypatch.setattr(subprocess, "call", lambda cmd, **kw: 7)
    with pytest.raises(RuntimeError):
        pipeline.pcaCall({"data-folder": "ds", "training-set-size": -1, "state-dim": 3})


@pytest.mark.parametrize("case", pu.CASES, ids=pu.case_name)
def test_rebuilt_object_transforms_on_the_host(kats, case):
    """components_ and mean_ as recorded from sklearn -> the recorded states, from uint8 planar and from float frames, before and after
    a pickle round trip; no GPU, no device tensor in the pickle."""
    from srl_baselines.ipca import IncrementalPCA, hostLut
    name = pu.case_name(case)
    assert np.array_equal(hostLut(), kats["lut"])
    frames, want = kats[name + "/frames"], kats[name + "/final/states"]
    ipca = IncrementalPCA.fromAttributes(components_=kats[name + "/final/components_"], mean_=kats[name + "/final/mean_"])
    tol = pu.tolerance(pu.load_spread()[name]) * np.abs(want).max()
    again = pickle.loads(pickle.dumps(ipca))
    for obj in (ipca, again):
        for x in (frames, pu.normalised(frames, kats["lut"]).astype(np.float32)):
            got = obj.transform(x)
            assert got.shape == want.shape and got.dtype == np.float32
            assert np.abs(got - want).max() <= tol
    assert again.n_components_ == case[5] and again.components_.shape == (case[5], frames[0].size)
    with pytest.raises(ValueError):
        ipca.transform(np.zeros((2, 5), dtype=np.float32))
    with pytest.raises(RuntimeError):  # an object without device state cannot be fitted further (and never on the host)
        again.partial_fit(frames)


def test_fitting_without_a_gpu_raises_the_no_cpu_path_error(monkeypatch, kats):
    import torch as th
    from srl_baselines.ipca import IncrementalPCA
    from srl_baselines import pca
    monkeypatch.setattr(th.cuda, "is_available", lambda: False)
    frames = th.from_numpy(kats[pu.case_name(pu.CASES[0]) + "/frames"][:4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IncrementalPCA(3).partial_fit(frames)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pca.fitAndTransform(np.array(["ds/record_000/frame000000"]), 3, 16)
    with pytest.raises(AttributeError):
        IncrementalPCA(3).components_


def test_eigenpairs_of_a_rank_deficient_gram_matrix_give_zero_rows():
    """Fewer distinct frames than components: the missing singular values are zero, their rows of W are zero — no division by zero."""
    from srl_baselines.ipca import leadingEigenpairs
    rs = np.random.RandomState(0)
    A = np.vstack([rs.randn(2, 50)] * 3)  # 6 rows, rank 2
    S, W, zeroed = leadingEigenpairs(A.dot(A.T), 4, 50)
    assert zeroed == 2 and S.shape == (6,) and (S[2:] == 0).all() and (S[:2] > 0).all()
    assert (W[2:] == 0).all() and np.allclose(np.linalg.norm(W[:2], axis=1), 1.0)
    assert np.allclose(S[:2], np.linalg.svd(A, compute_uv=False)[:2], rtol=1e-12)


def test_abi_declares_exports_and_binds_the_pca_entry_points(cabi):
    import ctypes
    declared = declared_symbols()
    lib = ctypes.CDLL(cabi.LIB_PATH)
    for s in ENTRY_POINTS:
        assert s in declared, "include/srlz.h does not declare " + s
        assert hasattr(lib, s), "libsrlz_hip.so does not export " + s
        assert s in cabi.EXPORTED, "srlz/_cabi.py has no prototype for " + s
    assert cabi.version() == cabi.ABI_VERSION == 104  # additive change


def test_workspace_queries_and_rejections_on_the_host(cabi):
    """Shape logic that needs no GPU: every rejection happens before any launch."""
    assert cabi.pca_workspace(20, 150528) > 0 and cabi.pca_workspace(0, 100) == 0 and cabi.pca_workspace(8, 0) == 0
    # [tiles][chunks][16][16] fp64: one tile, one chunk for D <= 256
    assert cabi.pca_workspace(8, 189) == 256 * 8 and cabi.pca_workspace(22, 189) == 3 * 256 * 8
    assert cabi.pca_transform_workspace(37, 3, 189) == 3 * 256 * 8 and cabi.pca_transform_workspace(0, 3, 189) == 0
    one = cabi.c_void_p(16)  # never dereferenced: the launchers reject first
    for what, rc in (("m < 1", cabi._lib.srlz_pca_stats(None, one, None, 1, 0, 10, 0, one, one, one, one, None)),
                     ("k > m first", cabi._lib.srlz_pca_gram(None, 5, 1, None, one, None, 1, 4, one, None, 10, one, one, 1 << 20, None)),
                     ("k > D", cabi._lib.srlz_pca_gram(one, 11, 0, None, one, None, 1, 12, one, one, 10, one, one, 1 << 20, None)),
                     ("k > D project", cabi._lib.srlz_pca_project(one, one, 11, 0, None, one, None, 1, 12, one, one, 10, one, None)),
                     ("m < 1 transform", cabi._lib.srlz_pca_transform(None, one, None, 1, 0, one, one, one, 3, 10, one, one, 1 << 20, None))):
        assert rc == -1, what
        assert cabi.error_text(), what
    assert cabi._lib.srlz_pca_gram(one, 3, 0, None, one, None, 1, 4, one, one, 10, one, one, 8, None) == -2  # short workspace
    assert "workspace" in cabi.error_text()
    assert cabi._lib.srlz_pca_project(one, one, 3, 0, None, one, None, 1, 4, one, one, 10, one, None) == -1  # out is the basis read
    assert cabi._lib.srlz_pca_stats(one, one, None, 1, 4, 10, 0, one, one, one, one, None) == -4  # both frame forms given


@pytest.mark.skipif(not os.path.exists(isa_audit.HIPCC) and shutil.which("hipcc") is None, reason="needs hipcc")
def test_pca_kernels_have_no_spills_and_no_serialised_stores():
    ks = list(isa_audit.kernels(isa_audit.disassemble(os.path.join(isa_audit.CSRC, "pca.hip"))))
    names = isa_audit.demangle([k for k, _ in ks])
    audits = {name: isa_audit.audit(body) for (_, body), name in zip(ks, names)}
    mfma = [n for n in audits if n.startswith(("pca_tiles_kernel", "pca_project_kernel"))]
    assert len(mfma) == 5, sorted(audits)  # four instantiations of the tile kernel (vector loads or not, triangle or rectangle)
    for name in mfma:
        a = audits[name]
        assert a["mfma"] > 0, name
        assert a["scratch_reloads"] == 0, "%s spills (%d scratch reloads)" % (name, a["scratch_reloads"])
        assert a["store_wait_chain"] == 0, "%s: a store waits for the one before it" % name
    for name, a in audits.items():
        assert a["store_wait_chain"] < 2, "%s: %d stores each wait for the previous one" % (name, a["store_wait_chain"] + 1)
