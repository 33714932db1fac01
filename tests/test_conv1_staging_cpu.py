"""srlz_conv1_buffer_staging_supported (host only, launches nothing): which conv1 descriptors take the buffer staging of the image
window (csrc/skinny.hip: image_request_buf) and which keep the generic-pointer staging."""
import pytest


@pytest.fixture(scope="module")
def C():
    from srlz import _cabi
    return _cabi


def conv1_desc(C, n, c, h, w, groups=1):
    return C.SkinnyDesc(n, c, h, w, (h - 1) // 2 + 1, (w - 1) // 2 + 1, 0, groups)


def test_the_step_takes_the_buffer_staging(C):
    # the headline step: 2 x 256 frames of 3 x 224 x 224 in two BatchNorm groups — floats and uint8 frames share the descriptor
    assert C.conv1_buffer_staging_supported(conv1_desc(C, 512, 3, 224, 224, 2)) == 1
    assert C.conv1_buffer_staging_supported(conv1_desc(C, 512, 3, 224, 224, 1)) == 1
    assert C.conv1_buffer_staging_supported(conv1_desc(C, 2, 3, 64, 64)) == 1


def test_a_tensor_beyond_a_resource_keeps_the_generic_staging(C):
    # 7133 float frames of 3 x 224 x 224 are the last to stay below 2^32 bytes
    assert 7133 * 3 * 224 * 224 * 4 < 2 ** 32 <= 7134 * 3 * 224 * 224 * 4
    assert C.conv1_buffer_staging_supported(conv1_desc(C, 7000, 3, 224, 224)) == 1
    assert C.conv1_buffer_staging_supported(conv1_desc(C, 7134, 3, 224, 224)) == 0
    assert C.conv1_buffer_staging_supported(conv1_desc(C, 8192, 3, 224, 224)) == 0
    # one image plane of 2^24 bytes or more (the offsets inside a window are 24-bit products)
    assert C.conv1_buffer_staging_supported(conv1_desc(C, 1, 3, 2048, 2048)) == 0


def test_other_shapes_keep_the_generic_staging(C):
    assert C.conv1_buffer_staging_supported(conv1_desc(C, 4, 6, 224, 224)) == 0    # two channel triples (MULTI)
    assert C.conv1_buffer_staging_supported(conv1_desc(C, 4, 9, 224, 224)) == 0
    assert C.conv1_buffer_staging_supported(C.SkinnyDesc(4, 3, 224, 224, 111, 111, 1, 1)) == 0   # K = 4: the last ConvTranspose
