#!/usr/bin/env python
"""Cost of the picture kernels of csrc/latent.hip on one GPU: python tools/kb_enjoy.py [--out profiles/kb_enjoy.json]

Per shape (n, w, h, cols): srlz_decoded_to_sheet_u8 and srlz_decoded_to_bgr on resident buffers, HIP events over warmed-up
repetitions, every timed window at least --window seconds long.  The calls walk a ring of input / output buffers larger than the
256 MB last-level cache, so no call finds its input there.  Rates are over the ALGORITHMIC bytes: per pixel 12 read and 3 written for
the sheet (its background bytes are counted too), 12 read and 12 written for the float images.  Prints one JSON object and writes it
to --out.  The numbers are for the record, not a gate: a default sheet is one launch of a few tens of microseconds."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "srl-zoo_amd"))

# the default sheet of a 4-dimensional block (--steps 11), a 200-dimensional one cut at MAX_BATCH_SIZE_GPU pictures
SHAPES = [(44, 224, 224, 11), (256, 224, 224, 16)]
GAP = 2
RING_BYTES = 768 << 20


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kb_enjoy.json"))
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kb_enjoy measures on a GPU"
    from srlz import _cabi as C, ops
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "gap": GAP, "ring_bytes": RING_BYTES, "shapes": []}
    for n, w, h, cols in SHAPES:
        sh, sw = ops.sheet_size(n, w, h, cols, GAP)
        in_bytes, sheet_bytes, img_bytes = 12 * n * w * h, 3 * sh * sw, 12 * n * w * h
        ring = max(2, -(-RING_BYTES // (in_bytes + img_bytes)))
        gen = torch.Generator(device=dev).manual_seed(0)
        decs = [torch.randn((n, 3, w, h), device=dev, generator=gen) for _ in range(ring)]
        sheets = [torch.empty((sh, sw, 3), dtype=torch.uint8, device=dev) for _ in range(ring)]
        imgs = [torch.empty((n, h, w, 3), dtype=torch.float32, device=dev) for _ in range(ring)]
        turn = [0]

        def sheet():
            k = turn[0] = (turn[0] + 1) % ring
            C.decoded_to_sheet_u8(C.ptr(decs[k]), n, w, h, cols, GAP, 255, 1, C.ptr(sheets[k]), sh, sw, C.stream())

        def bgr():
            k = turn[0] = (turn[0] + 1) % ring
            C.decoded_to_bgr(C.ptr(decs[k]), n, w, h, C.ptr(imgs[k]), C.stream())
        sheet_ms, sheet_reps = timed_window(sheet, args.window)
        bgr_ms, bgr_reps = timed_window(bgr, args.window)
        rec = {"n": n, "w": w, "h": h, "cols": cols, "sheet_h": sh, "sheet_w": sw, "ring": ring,
               "sheet_ms": sheet_ms, "sheet_reps": sheet_reps, "sheet_algorithmic_bytes": in_bytes + sheet_bytes,
               "sheet_gbps": (in_bytes + sheet_bytes) / (sheet_ms * 1e-3) / 1e9,
               "bgr_ms": bgr_ms, "bgr_reps": bgr_reps, "bgr_algorithmic_bytes": in_bytes + img_bytes,
               "bgr_gbps": (in_bytes + img_bytes) / (bgr_ms * 1e-3) / 1e9}
        res["shapes"].append(rec)
        print(json.dumps(rec))
        del decs, sheets, imgs
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
