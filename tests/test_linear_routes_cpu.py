"""The route of every nn.Linear GEMM (csrc/linear.hip), asked from the host: srlz_linear_debug_route reports the plan that the five entry
points execute — kernel, number of reduction chunks nz, chunk length rchunk — without launching anything, so this file needs no GPU.

Three kinds of checks: hand-pinned rows (a regression pin read off vec_ok / choose_splits, not a specification), properties every plan
has to have whatever the heuristics become (the chunks tile the reduction, fit the workspace, are whole kernel steps; a misaligned
operand never reaches the 16-byte loads), and a replay of the vectorisation predicate in Python which shows that the three directions
reach gemm_vec_kernel<0,0>, <0,1> and <1,1> and never <1,0> — the reason that instantiation does not exist.
tests/test_linear_kernels_gpu.py imports `route` and asserts its cases' routes with it before it launches them."""
import ctypes
import itertools

import pytest

FWD, BWD_DATA, BWD_WEIGHT = 0, 1, 2
STRIDED, VEC_RR, VEC_RJ, VEC_IJ = 0, 1, 2, 3  # gemm_strided_kernel, gemm_vec_kernel<0,0>, <0,1>, <1,1>
KERNEL_NAME = {STRIDED: "strided", VEC_RR: "vec00", VEC_RJ: "vec01", VEC_IJ: "vec11"}
STEP = {STRIDED: 32, VEC_RR: 64, VEC_RJ: 64, VEC_IJ: 64}
ALIGNED = 0x7f0000001000  # an address that is never dereferenced
DEFAULT = "default"

SIZES = list(range(1, 70)) + [128, 200, 206, 400, 512, 516, 2304]


def gemm_shape(op, M, N, K, Kout=None):
    """(I, J, R) of the GEMM behind an entry point: the result is I x J, the reduction R long."""
    if op == FWD:
        return M, N, K
    if op == BWD_DATA:
        return M, (K if Kout is None else Kout), N
    return N, K, M


def route(cabi, op, M, N, K, Kout=None, a=ALIGNED, b=ALIGNED, ws_bytes=DEFAULT):
    """(kernel, nz, rchunk).  ws_bytes: DEFAULT = srlz_linear_workspace(M, N, K) as srlz.ops passes it, None = no workspace."""
    out = (ctypes.c_int * 3)(-1, -1, -1)
    if ws_bytes == DEFAULT:
        ws_bytes = cabi.linear_workspace(M, N, K)
    has_ws = ws_bytes is not None
    cabi.linear_debug_route(op, M, N, K, K if Kout is None else Kout, ctypes.c_void_p(a), ctypes.c_void_p(b), int(has_ws),
                            ws_bytes if has_ws else 0, out)
    return out[0], out[1], out[2]


@pytest.mark.parametrize("op,M,N,K,kernel,nz,rchunk", [
    (FWD, 256, 200, 2304, VEC_RR, 12, 192),        # the encoder's FC layer at batch 256
    (BWD_DATA, 256, 200, 2304, VEC_RJ, 1, None),
    (BWD_WEIGHT, 256, 200, 2304, VEC_IJ, 1, None),
    (BWD_DATA, 512, 2304, 200, VEC_RJ, 12, 192),   # the decoder's FC layer, both frames as one batch
    (FWD, 3, 200, 206, STRIDED, 1, None),          # the forward model: K = 206 is no multiple of 4
    (BWD_WEIGHT, 512, 6, 400, STRIDED, 4, 128),    # the inverse head's dw in a batch-256 step
    (BWD_WEIGHT, 512, 200, 206, STRIDED, 4, 128),  # the forward model's dw in a batch-256 step
    (FWD, 64, 64, 516, VEC_RR, 3, 192),            # 4 splits asked for, 3 chunks after rounding up to a step
    (FWD, 64, 64, 515, STRIDED, 4, 160),
    (FWD, 64, 64, 508, VEC_RR, 1, None),
    (FWD, 64, 64, 640, VEC_RR, 5, 128),
])
def test_pinned_routes(cabi, op, M, N, K, kernel, nz, rchunk):
    got = route(cabi, op, M, N, K)
    R = gemm_shape(op, M, N, K)[2]
    assert got == (kernel, nz, R if rchunk is None else rchunk)


def test_workspace_size_limits_the_split(cabi):
    assert route(cabi, FWD, 64, 64, 2304) == (VEC_RR, 12, 192)
    assert route(cabi, FWD, 64, 64, 2304, ws_bytes=5 * 64 * 64 * 4) == (VEC_RR, 5, 512)
    assert route(cabi, FWD, 64, 64, 2304, ws_bytes=2 * 64 * 64 * 4 - 1) == (VEC_RR, 1, 2304)
    assert route(cabi, FWD, 64, 64, 2304, ws_bytes=None) == (VEC_RR, 1, 2304)


# ---- the vectorisation predicate, replayed -------------------------------------------------------------------------------------
def operand_layout(addr, s_row, s_r, nrow, R):
    """None, or whether an operand whose (row, r) element sits at row * s_row + r * s_r is contiguous along its row index: the 16-byte
    loads need an aligned base, a reduction of whole float4s, and whole aligned float4s along whichever index is contiguous."""
    if addr % 16 or R % 4:
        return None
    if s_r == 1 and s_row % 4 == 0:
        return False
    if s_row == 1 and s_r % 4 == 0 and nrow % 4 == 0:
        return True
    return None


def replay_kernel(op, M, N, K, Kout=None, a=ALIGNED, b=ALIGNED):
    """The kernel by the header comment of linear.hip: (stride of A along i, along r), (of B along j, along r) per direction.  Returns
    "vec10" for the combination that has no kernel."""
    I, J, R = gemm_shape(op, M, N, K, Kout)
    (sai, sar), (sbj, sbr) = {FWD: ((K, 1), (K, 1)), BWD_DATA: ((N, 1), (1, K)), BWD_WEIGHT: ((1, N), (1, K))}[op]
    ai, bi = operand_layout(a, sai, sar, I, R), operand_layout(b, sbj, sbr, J, R)
    if ai is None or bi is None:
        return STRIDED
    return {(False, False): VEC_RR, (False, True): VEC_RJ, (True, True): VEC_IJ, (True, False): "vec10"}[(ai, bi)]


def test_plan_properties_and_reachable_kernels(cabi):
    """Every plan over M, N, K in [1, 69] and the model's sizes, all three directions, with the default workspace."""
    lib_route = cabi._lib.srlz_linear_debug_route
    out = (ctypes.c_int * 3)()
    aligned = ctypes.c_void_p(ALIGNED)
    reached = {FWD: set(), BWD_DATA: set(), BWD_WEIGHT: set()}
    vec_cases = []
    for M, N, K in itertools.product(SIZES, repeat=3):
        ws_bytes = 16 * 4 * max(M * N, M * K, N * K)
        for op in (FWD, BWD_DATA, BWD_WEIGHT):
            assert lib_route(op, M, N, K, K, aligned, aligned, 1, ws_bytes, out) == 0
            kernel, nz, rchunk = out[0], out[1], out[2]
            I, J, R = gemm_shape(op, M, N, K)
            case = (op, M, N, K)
            assert kernel == replay_kernel(op, M, N, K), case
            assert nz >= 1, case
            assert (nz - 1) * rchunk < R <= nz * rchunk, case
            assert nz == 1 or rchunk % STEP[kernel] == 0, case
            assert nz * I * J * 4 <= ws_bytes, case
            reached[op].add(kernel)
            if kernel != STRIDED and len(vec_cases) < 4000:
                vec_cases.append(case)
    assert reached == {FWD: {STRIDED, VEC_RR}, BWD_DATA: {STRIDED, VEC_RJ}, BWD_WEIGHT: {STRIDED, VEC_IJ}}
    assert cabi.linear_workspace(5, 7, 3) == 16 * 4 * 35 and cabi.linear_workspace(2, 3, 9) == 16 * 4 * 27
    # an operand that does not start on a 16-byte boundary takes the dword kernel, whichever operand and offset it is
    for op, M, N, K in vec_cases:
        for off in (4, 8, 12):
            assert route(cabi, op, M, N, K, a=ALIGNED + off)[0] == STRIDED, (op, M, N, K, "a", off)
            assert route(cabi, op, M, N, K, b=ALIGNED + off)[0] == STRIDED, (op, M, N, K, "b", off)


def test_small_workspaces_and_partial_data_gradients(cabi):
    """The same properties where the workspace, not the tile count, limits the split, and for Kout < K."""
    for op, M, N, K in [(FWD, 64, 64, 2304), (FWD, 63, 65, 2303), (BWD_DATA, 64, 2304, 64), (BWD_DATA, 5, 515, 9),
                        (BWD_WEIGHT, 2304, 64, 64), (BWD_WEIGHT, 516, 6, 400), (BWD_WEIGHT, 515, 200, 206)]:
        I, J, R = gemm_shape(op, M, N, K)
        one = I * J * 4
        for ws_bytes in [0, 1, one, 2 * one - 1, 2 * one, 3 * one + 5, 5 * one, 15 * one, 16 * one, 100 * one]:
            kernel, nz, rchunk = route(cabi, op, M, N, K, ws_bytes=ws_bytes)
            assert kernel == replay_kernel(op, M, N, K)
            assert nz >= 1 and (nz - 1) * rchunk < R <= nz * rchunk
            assert nz == 1 or (rchunk % STEP[kernel] == 0 and nz * one <= ws_bytes), (op, M, N, K, ws_bytes)
        assert route(cabi, op, M, N, K, ws_bytes=None)[1:] == (1, R)
    for M, N, K, Kout in [(5, 64, 72, 68), (65, 128, 136, 64), (3, 200, 206, 200), (65, 10, 14, 10), (5, 64, 72, 1), (4, 512, 72, 68),
                          (4, 512, 72, 67), (4, 515, 72, 68)]:
        kernel, nz, rchunk = route(cabi, BWD_DATA, M, N, K, Kout)
        assert kernel == replay_kernel(BWD_DATA, M, N, K, Kout)
        assert nz >= 1 and (nz - 1) * rchunk < N <= nz * rchunk and (nz == 1 or rchunk % STEP[kernel] == 0)
        assert nz * M * Kout * 4 <= cabi.linear_workspace(M, N, K)
    # J = Kout columns of a K-wide w: w is contiguous along j, so the vector route needs whole float4s of columns, Kout % 4 == 0
    # (Kout = 1 is a strided case whatever K is)
    assert route(cabi, BWD_DATA, 5, 64, 72, 68)[0] == VEC_RJ and route(cabi, BWD_DATA, 65, 128, 136, 64)[0] == VEC_RJ
    assert route(cabi, BWD_DATA, 5, 64, 72, 66)[0] == STRIDED and route(cabi, BWD_DATA, 5, 64, 72, 1)[0] == STRIDED
    assert route(cabi, BWD_DATA, 3, 200, 206, 200)[0] == STRIDED


def test_no_direction_states_a_gemm_for_vec10():
    """A contiguous along i next to B contiguous along r has no kernel (gemm_vec_kernel<1,0> is not instantiated; the plan would send it
    to the strided kernel).  A runs along i only in the weight gradient, and there B = x runs along j or is not vectorisable."""
    for op in (FWD, BWD_DATA, BWD_WEIGHT):
        for M, N, K in itertools.product(range(1, 70), repeat=3):
            assert replay_kernel(op, M, N, K) != "vec10"
            if op == BWD_DATA:
                for Kout in {1, max(1, K - 4), max(1, K - 1)}:
                    assert replay_kernel(op, M, N, K, Kout) != "vec10"


@pytest.mark.parametrize("args,text", [
    ((BWD_DATA, 4, 4, 4, 0), "input columns"),
    ((BWD_DATA, 4, 4, 4, 5), "input columns"),
    ((FWD, 0, 4, 4, 4), "empty GEMM"),
    ((FWD, 4, 0, 4, 4), "empty GEMM"),
    ((BWD_WEIGHT, 4, 4, 0, 0), "empty GEMM"),
    ((BWD_DATA, 4, 0, 4, 4), "empty GEMM"),
    ((3, 4, 4, 4, 4), "unknown op"),
    ((-1, 4, 4, 4, 4), "unknown op"),
])
def test_bad_arguments_are_rejected(cabi, args, text):
    out = (ctypes.c_int * 3)(-7, -7, -7)
    rc = cabi._lib.srlz_linear_debug_route(*args, ctypes.c_void_p(ALIGNED), ctypes.c_void_p(ALIGNED), 1, 1 << 20, out)
    assert rc < 0 and text in cabi.error_text()
    assert list(out) == [-7, -7, -7]
    with pytest.raises(cabi.SrlzError):
        cabi.linear_debug_route(*args, ctypes.c_void_p(ALIGNED), ctypes.c_void_p(ALIGNED), 1, 1 << 20, out)
    # the other directions do not look at Kout
    assert cabi._lib.srlz_linear_debug_route(FWD, 4, 4, 4, 0, ctypes.c_void_p(ALIGNED), ctypes.c_void_p(ALIGNED), 0, 0, out) == 0
    assert list(out) == [VEC_RR, 1, 4]
