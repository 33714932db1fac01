"""srlz_decoded_to_bgr / srlz_decoded_to_sheet_u8 (csrc/latent.hip) through the C ABI against their numpy restatements
(tests/enjoy_util.py): bit for bit, no tolerance.

Shapes (n, w, h): one pixel; maps smaller than a tile with w != h both ways; a map that is no multiple of the 32 x 64 tile in either
direction and spans several tiles; one whole tile row; the product's 224 x 224 with two images.  Inputs are scaled so that about a
fifth of the values clip at each end, with values that land on exactly 0 and exactly 1 among them."""
import numpy as np
import pytest
import torch

import enjoy_util as eu

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 3, 5), (2, 5, 3), (3, 33, 65), (1, 64, 64), (2, 224, 224)]
SENTINEL = 77.0
SENTINEL_U8 = 77
TAIL = 64
DEV = "cuda"

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def decoded_input(n, w, h):
    """[n, 3, w, h] float32: de-normalised values uniform on [-0.33, 1.33] (a fifth below 0, a fifth above 1).  Every plane with room
    for them also holds, for the ends 0 and 1 of the clip, the five floats around (goal - mean) / std: their de-normalised values
    straddle the end and land on it exactly where fl(fl(x * std) + mean) can (it cannot give 0 in the green channel).
    :return: (dec, number of planted values whose UNCLIPPED result is exactly 0, the same for exactly 1)"""
    rs = np.random.RandomState(1000 * n + 10 * w + h)
    target = rs.uniform(-1.0 / 3, 4.0 / 3, (n, 3, w, h)).astype(np.float32)
    dec = ((target - MEAN[None, :, None, None]) / STD[None, :, None, None]).astype(np.float32)
    exact = [0, 0]
    if w * h >= 10:
        flat = dec.reshape(n, 3, -1)
        for c in range(3):
            for k, goal in enumerate((np.float32(0), np.float32(1))):
                x0 = np.float32((goal - MEAN[c]) / STD[c])
                for j, d in enumerate(range(-2, 3)):
                    x = np.float32(x0 + np.float32(d) * np.spacing(x0))
                    flat[:, c, 5 * k + j] = x
                    exact[k] += int(np.float32(np.float32(x * STD[c]) + MEAN[c]) == goal)
    return dec, exact[0], exact[1]


@pytest.fixture(scope="module")
def problems():
    """Per shape: the input, its device copy, the numpy image — computed once, shared and never written."""
    out = {}
    for n, w, h in SHAPES:
        dec, exact0, exact1 = decoded_input(n, w, h)
        ref = eu.numpy_bgr(dec)
        ref.setflags(write=False)
        out[(n, w, h)] = (dec, torch.from_numpy(dec).to(DEV), ref, (exact0, exact1))
    return out


def test_inputs_clip_at_both_ends(problems):
    for (n, w, h), (dec, _, ref, exact) in problems.items():
        if w * h >= 10:
            assert exact[0] >= 2 and exact[1] >= 3, (n, w, h, exact)  # exactly 0 / exactly 1 before the clip
            assert (ref == 0).any() and (ref == 1).any()
            # the planted neighbours straddle both ends: some survive the clip just inside
            assert ((ref > 0) & (ref < 1e-6)).any() and ((ref < 1) & (ref > 1 - 1e-6)).any()
        if n * w * h >= 1000:
            assert 0.15 < (ref == 0).mean() < 0.25 and 0.15 < (ref == 1).mean() < 0.25
            inner = ref[(ref > 0) & (ref < 1)]
            assert inner.size > 0.5 * ref.size


def _bgr(cabi, dec_d, n, w, h):
    whole = torch.full((n * h * w * 3 + TAIL,), SENTINEL, dtype=torch.float32, device=DEV)
    cabi.decoded_to_bgr(cabi.ptr(dec_d), n, w, h, cabi.ptr(whole), cabi.stream())
    torch.cuda.synchronize()
    return whole


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_w%d_h%d" % s)
def test_decoded_to_bgr_bit_for_bit(cabi, problems, shape):
    n, w, h = shape
    dec, dec_d, ref, _ = problems[shape]
    whole = _bgr(cabi, dec_d, n, w, h).cpu().numpy()
    got = whole[:n * h * w * 3].reshape(n, h, w, 3)
    assert got.tobytes() == ref.tobytes(), "%d of %d values differ, largest difference %g" % (
        (got != ref).sum(), ref.size, np.abs(got - ref).max())
    assert (whole[n * h * w * 3:] == SENTINEL).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_w%d_h%d" % s)
def test_decoded_to_sheet_byte_for_byte(cabi, problems, shape):
    n, w, h = shape
    dec, dec_d, ref, _ = problems[shape]
    img = _bgr(cabi, dec_d, n, w, h)[:n * h * w * 3].cpu().numpy().reshape(n, h, w, 3)  # the device's own float images
    for cols in sorted({1, 2, n, n + 1}):
        for gap in (0, 2):
            for rgb in (0, 1):
                for fill in (0, 255):
                    want = eu.numpy_sheet(img, cols, gap, fill, rgb)
                    sh, sw = want.shape[:2]
                    other = 128  # neither fill: a byte nobody wrote shows up wherever the sheet should be fill (pictures: below)
                    whole = torch.full((sh * sw * 3 + TAIL,), other, dtype=torch.uint8, device=DEV)
                    whole[sh * sw * 3:] = SENTINEL_U8
                    cabi.decoded_to_sheet_u8(cabi.ptr(dec_d), n, w, h, cols, gap, fill, rgb, cabi.ptr(whole), sh, sw, cabi.stream())
                    torch.cuda.synchronize()
                    got = whole.cpu().numpy()
                    what = "cols=%d gap=%d rgb=%d fill=%d" % (cols, gap, rgb, fill)
                    assert got[:sh * sw * 3].tobytes() == want.tobytes(), what
                    assert (got[sh * sw * 3:] == SENTINEL_U8).all(), what


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_w%d_h%d" % s)
def test_sheet_writes_every_byte(cabi, problems, shape):
    """Pre-fill with a third value the result cannot hold anywhere (pictures that clip to 0 or 1 only, so bytes 0 / 255, and fill
    255): none of it is left, and a call over another pre-fill gives the same bytes."""
    n, w, h = shape
    dec = np.where(problems[shape][0] > 0, np.float32(50), np.float32(-50)).astype(np.float32)
    dec_d = torch.from_numpy(dec).to(DEV)
    cols, gap = 2, 2
    rows = (n + cols - 1) // cols
    sh, sw = rows * h + (rows + 1) * gap, cols * w + (cols + 1) * gap
    results = []
    for prefill in (7, 9):
        sheet = torch.full((sh, sw, 3), prefill, dtype=torch.uint8, device=DEV)
        cabi.decoded_to_sheet_u8(cabi.ptr(dec_d), n, w, h, cols, gap, 255, 1, cabi.ptr(sheet), sh, sw, cabi.stream())
        torch.cuda.synchronize()
        got = sheet.cpu().numpy()
        assert set(np.unique(got)) <= {0, 255}, np.unique(got)
        results.append(got)
    assert np.array_equal(results[0], results[1])
    if n % cols:
        assert (results[0][sh - gap - h:, sw - gap - w:] == 255).all()  # the empty tile of the last row


def test_rejected_arguments_launch_nothing(cabi):
    lib = cabi._lib
    n, w, h = 2, 5, 3
    dec = torch.zeros((n, 3, w, h), dtype=torch.float32, device=DEV)
    sh, sw = h + 4, 2 * w + 6
    sheet = torch.full((sh, sw, 3), 9, dtype=torch.uint8, device=DEV)
    img = torch.full((n, h, w, 3), SENTINEL, dtype=torch.float32, device=DEV)
    d, s, i, st = cabi.ptr(dec), cabi.ptr(sheet), cabi.ptr(img), cabi.stream()
    BAD, NULL = -1, -4
    assert lib.srlz_decoded_to_sheet_u8(d, n, w, h, 2, 2, 255, 1, s, sh + 1, sw, st) == BAD      # wrong sheet size
    assert lib.srlz_decoded_to_sheet_u8(d, n, w, h, 2, 2, 255, 1, s, sh, sw - 1, st) == BAD
    assert lib.srlz_decoded_to_sheet_u8(d, n, w, h, 1, 2, 255, 1, s, sh, sw, st) == BAD          # the size of another grid
    assert lib.srlz_decoded_to_sheet_u8(d, 0, w, h, 2, 2, 255, 1, s, sh, sw, st) == BAD          # n = 0
    assert lib.srlz_decoded_to_bgr(d, 0, w, h, i, st) == BAD
    assert lib.srlz_decoded_to_sheet_u8(d, n, w, h, 2, 2, 256, 1, s, sh, sw, st) == BAD          # fill = 256
    assert lib.srlz_decoded_to_sheet_u8(d, n, w, h, 2, 2, -1, 1, s, sh, sw, st) == BAD
    assert lib.srlz_decoded_to_sheet_u8(d, n, w, h, 2, -1, 255, 1, s, sh, sw, st) == BAD
    assert lib.srlz_decoded_to_sheet_u8(d, n, w, h, 0, 2, 255, 1, s, sh, sw, st) == BAD
    assert lib.srlz_decoded_to_sheet_u8(None, n, w, h, 2, 2, 255, 1, s, sh, sw, st) == NULL      # null pointers
    assert lib.srlz_decoded_to_sheet_u8(d, n, w, h, 2, 2, 255, 1, None, sh, sw, st) == NULL
    assert lib.srlz_decoded_to_bgr(None, n, w, h, i, st) == NULL
    assert lib.srlz_decoded_to_bgr(d, n, w, h, None, st) == NULL
    # the 2^31 limits by arithmetic on the descriptor (the buffers behind the pointers are the small ones above: a launch would be
    # out of bounds, which is why the check must come first): 3 * 2^31 floats of input; a sheet of 4.58e9 bytes from 48 floats
    assert (1 << 15) * 3 * (1 << 8) * (1 << 8) >= 2 ** 31
    assert lib.srlz_decoded_to_bgr(d, 1 << 15, 1 << 8, 1 << 8, i, st) == BAD
    big_h, big_w = 2 * 6700 + 1, 17 * 6700 + 16
    assert big_h * big_w * 3 >= 2 ** 31
    assert lib.srlz_decoded_to_sheet_u8(d, 16, 1, 1, 16, 6700, 255, 1, s, big_h, big_w, st) == BAD
    assert "2^31" in cabi.error_text()
    torch.cuda.synchronize()
    assert bool((sheet == 9).all()) and bool((img == SENTINEL).all())


def test_ops_wrappers(problems):
    from srlz import ops
    from srlz._cabi import SrlzError
    n, w, h = 3, 33, 65
    dec, dec_d, ref, _ = problems[(n, w, h)]
    img = ops.decoded_to_bgr(dec_d)
    assert img.dtype == torch.float32 and tuple(img.shape) == (n, h, w, 3) and img.cpu().numpy().tobytes() == ref.tobytes()
    # a non-contiguous view goes through _check's contiguous()
    assert ops.decoded_to_bgr(dec_d.transpose(2, 3)).cpu().numpy().tobytes() == eu.numpy_bgr(dec.transpose(0, 1, 3, 2)).tobytes()
    sheet = ops.decoded_to_sheet(dec_d, cols=2)
    assert sheet.dtype == torch.uint8 and tuple(sheet.shape) == ops.sheet_size(n, w, h, 2, 2) + (3,)
    assert np.array_equal(sheet.cpu().numpy(), eu.numpy_sheet(ref, 2, 2, 255, True))
    assert np.array_equal(ops.decoded_to_sheet(dec_d, 3, gap=0, fill=0, rgb=False).cpu().numpy(), eu.numpy_sheet(ref, 3, 0, 0, False))
    for bad in (dec, dec_d.double(), dec_d[:, :2], torch.zeros((n, 6, w, h), device=DEV), dec_d[0]):
        with pytest.raises(SrlzError):
            ops.decoded_to_bgr(torch.from_numpy(bad) if isinstance(bad, np.ndarray) else bad)
    with pytest.raises(SrlzError):
        ops.decoded_to_sheet(dec_d, 0)
    with pytest.raises(SrlzError):
        ops.decoded_to_sheet(dec_d, 2, fill=256)
