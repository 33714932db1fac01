#!/usr/bin/env python
"""Cost of one minibatch of the PCA baseline (csrc/pca.hip, srl_baselines/ipca.py) on one GPU: python tools/kb_pca.py [--out profiles/kb_pca.json]

Per (k, bs) at D = 3 x 224 x 224 = 150 528, for a LATER minibatch (basis and correction row present, r = k + bs + 1 rows), on resident
planar uint8 frames:
  * each of the four entry points — srlz_pca_stats, srlz_pca_gram, srlz_pca_project, srlz_pca_transform (of the bs frames) — HIP
    events over warmed-up repetitions, every timed window at least --window seconds long; for the Gram matrix and the projection the
    fp64 operations the shapes imply (r (r + 1) D and 2 k r D) and the rate they give;
  * numpy.linalg.eigh of the r x r matrix on the host, and IncrementalPCA.partial_fit as a user calls it (device tensor in);
  * what the frames cost before they get here: decoding bs JPEG files of 224 x 224 with the loader's own reader, one thread;
  * sklearn's IncrementalPCA.partial_fit of the same later minibatch on the host (float32 frames, the threads the job may use), where
    sklearn imports (--no-ref skips it).
Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "srl-zoo_amd"))

SHAPES = [(3, 16), (200, 201)]  # (k, bs): the reference's default, and --state-dim 200 with its batch_size = max(k + 1, bs)
C3, W, H = 3, 224, 224


def timed_window(fn, window_s, warm=3):
    """Milliseconds per call over a window of at least window_s seconds (HIP events around the whole window)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    reps = max(5, int(np.ceil(window_s * 1e3 / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, reps


def host_ms(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def frames_u8(n, seed):
    """Smooth frames with some rank (as tests/dataset_util.py draws them) plus noise: n x [3, W, H] uint8."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:W, 0:H]
    out = np.empty((n, C3, W, H), dtype=np.uint8)
    for i in range(n):
        p = rs.rand(3)
        img = np.stack([127 + 100 * np.sin(xx / (20.0 + 30 * p[c]) + yy / (25.0 + 10 * c) + i * 0.1) for c in range(3)], 0)
        out[i] = np.clip(img + 4 * rs.randn(C3, W, H), 0, 255).astype(np.uint8)
    return out


def decode_ms_per_frame(frame_u8, reps=16):
    from PIL import Image
    from preprocessing.data_loader import _imread_rgb
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "frame.jpg")
        Image.fromarray(np.ascontiguousarray(frame_u8.transpose(2, 1, 0))).save(path, quality=95)
        _imread_rgb(path)
        t = time.perf_counter()
        for _ in range(reps):
            _imread_rgb(path)
        return (time.perf_counter() - t) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kb_pca.json"))
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--no-ref", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kb_pca measures on a GPU"
    from srlz import _cabi as C, ops
    from srl_baselines.ipca import IncrementalPCA, leadingEigenpairs
    dev = torch.device("cuda", 0)
    D = C3 * W * H
    res = {"D": D, "device": torch.cuda.get_device_name(0), "window_s": args.window, "shapes": []}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    for k, bs in SHAPES:
        host = frames_u8(2 * bs, seed=k)
        x0, x1 = torch.from_numpy(host[:bs]).to(dev), torch.from_numpy(host[bs:]).to(dev)
        ipca = IncrementalPCA(k).partial_fit(x0)  # the state a later minibatch finds
        d = ipca._dev
        r, m, n_seen = k + bs + 1, bs, bs
        lut, plane, s = C.ptr(ops.norm_lut(dev)), W * H, C.stream()
        mean, var = d["mean"].clone(), d["var"].clone()
        bmean, corr = torch.empty_like(mean), torch.empty_like(mean)
        basis, out = d["basis"][d["cur"]], torch.empty_like(d["basis"][0])
        nbytes, tbytes = C.pca_workspace(r, D), C.pca_transform_workspace(m, k, D)
        ws = torch.empty(max(nbytes, tbytes), dtype=torch.uint8, device=dev)
        G = torch.empty((r, r), dtype=torch.float64, device=dev)
        states = torch.empty((m, k), dtype=torch.float32, device=dev)

        def stats():
            mean.copy_(d["mean"])  # (in place: every repetition starts from the same state; the copies are 2 x 1.2 MB)
            var.copy_(d["var"])
            C.pca_stats(C.ptr(x1), None, lut, plane, m, D, n_seen, C.ptr(mean), C.ptr(var), C.ptr(bmean), C.ptr(corr), s)

        def gram():
            C.pca_gram(C.ptr(basis), k, 0, C.ptr(x1), None, lut, plane, m, C.ptr(bmean), C.ptr(corr), D, C.ptr(G), C.ptr(ws), nbytes, s)
        stats()
        gram()
        G_host = G.cpu().numpy()
        S_all, Wm, _ = leadingEigenpairs(G_host, k, D)
        W_dev = torch.from_numpy(Wm).to(dev)

        def project():
            C.pca_project(C.ptr(W_dev), C.ptr(basis), k, 0, C.ptr(x1), None, lut, plane, m, C.ptr(bmean), C.ptr(corr), D, C.ptr(out), s)

        def transform():
            C.pca_transform(C.ptr(x1), None, lut, plane, m, C.ptr(d["mean"]), C.ptr(basis), C.ptr(d["S"]), k, D, C.ptr(states),
                            C.ptr(ws), tbytes, s)
        rec = {"k": k, "bs": bs, "r": r, "gram_workspace_bytes": int(nbytes), "frame_bytes": int(x1.numel())}
        for name, fn in (("stats", stats), ("gram", gram), ("project", project), ("transform", transform)):
            ms, reps = timed_window(fn, args.window)
            rec[name + "_ms"], rec[name + "_reps"] = ms, reps
        rec["gram_fp64_ops"], rec["project_fp64_ops"] = float(r) * (r + 1) * D, 2.0 * k * r * D
        rec["gram_fp64_tflops"] = rec["gram_fp64_ops"] / (rec["gram_ms"] * 1e-3) / 1e12
        rec["project_fp64_tflops"] = rec["project_fp64_ops"] / (rec["project_ms"] * 1e-3) / 1e12
        rec["host_eigh_ms"] = host_ms(lambda: leadingEigenpairs(G_host, k, D))
        rec["G_download_ms"] = host_ms(lambda: G.cpu())
        again = IncrementalPCA(k).partial_fit(x0)

        def whole():
            again._dev["n"], again._dev["batches"] = bs, 1  # (every repetition is "the second minibatch")
            again.partial_fit(x1)
        rec["partial_fit_ms"] = host_ms(whole)
        rec["jpeg_decode_ms_per_frame_one_thread"] = decode_ms_per_frame(host[0])
        rec["jpeg_decode_ms_per_minibatch_one_thread"] = rec["jpeg_decode_ms_per_frame_one_thread"] * bs
        rec["sklearn_partial_fit_ms"] = None
        res["shapes"].append(rec)
        print(json.dumps(rec))
        save()
        del x0, x1, ws, ipca, again

    if not args.no_ref:
        try:
            import sklearn
            from sklearn.decomposition import IncrementalPCA as SkIPCA
            res["sklearn"] = sklearn.__version__
        except ImportError:
            SkIPCA, res["sklearn"] = None, None
        res["host_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count()
        from srl_baselines.ipca import hostLut
        lut = hostLut()
        for rec in res["shapes"]:
            if SkIPCA is None:
                continue
            k, bs = rec["k"], rec["bs"]
            host = frames_u8(2 * bs, seed=k)
            X = np.stack([lut[c][host[:, c]] for c in range(3)], axis=1).reshape(2 * bs, -1).astype(np.float32)
            p = SkIPCA(n_components=k).partial_fit(X[:bs].copy())
            t = time.perf_counter()
            p.partial_fit(X[bs:].copy())
            rec["sklearn_partial_fit_ms"] = (time.perf_counter() - t) * 1e3
            print(json.dumps({"k": k, "bs": bs, "sklearn_partial_fit_ms": rec["sklearn_partial_fit_ms"]}))
            save()
    print(json.dumps(res))
    save()


if __name__ == "__main__":
    main()
