"""The route table of the 64->64 convolution family, pinned: which virtual-grid program csrc/conv64.hip builds for a descriptor and
which kernels take it (the host-only answers of the C ABI; the route predicates sit next to their kernels, in csrc/conv64_pipe.hip and
csrc/conv64_wgrad.hip), against tests/golden/conv64_routes.json.  Host code only: no GPU.

The fixture was recorded with the library as it was BEFORE the route predicates were gathered in one place, so the test says that
gathering them changed no decision.  To record it again (only when a route is meant to change):  python tests/test_conv64_routes_cpu.py
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "conv64_routes.json")

# (hi, stride, pad, transposed): tests/test_programs.py::LAYERS
LAYERS = [(56, 1, 1, 0), (27, 2, 1, 0), (6, 2, 0, 1), (13, 2, 0, 1), (27, 2, 0, 1), (55, 2, 0, 1),
          (9, 1, 1, 0), (10, 2, 1, 0), (7, 2, 0, 1)]
# (hi, wi, stride, pad, transposed): the geometries of tests/test_rect_kernels_gpu.py::CONV64_RECT, each in both orientations
RECT = [(40, 56, 1, 1, 0), (19, 27, 2, 1, 0), (10, 14, 1, 1, 0), (4, 6, 2, 0, 1), (9, 13, 2, 0, 1), (19, 27, 2, 0, 1),
        (39, 55, 2, 0, 1), (9, 80, 1, 1, 0), (3, 8, 2, 1, 0), (3, 8, 2, 0, 1), (7, 12, 1, 1, 0), (1, 5, 1, 1, 0), (1, 5, 2, 0, 1),
        (2, 9, 2, 1, 0), (5, 25, 1, 1, 0), (8, 21, 2, 0, 0), (6, 11, 2, 1, 1)]
BATCHES = (2, 4, 32, 256, 512)
GROUPS = (1, 2)


def out_size(hi, s, p, t):
    return (hi - 1) * s - 2 * p + 3 if t else (hi + 2 * p - 3) // s + 1


def descriptors():
    shapes = [(hi, hi, s, p, t) for (hi, s, p, t) in LAYERS]
    for (hi, wi, s, p, t) in RECT:
        shapes += [(hi, wi, s, p, t), (wi, hi, s, p, t)]
    for (hi, wi, s, p, t) in shapes:
        for n in BATCHES:
            for g in GROUPS:
                if n % g == 0:
                    yield (n, hi, wi, s, p, t, g)


ROUTE_KEYS = ("fwd_tiles", "bwd_data_tiles", "gather_pipe_fwd", "gather_pipe_bwd", "bwd_fused", "bwd_fused_bn_rows")


def record(cabi):
    """{"programs": {shape: [forward dump, data-gradient dump]}, "routes": {descriptor: the ROUTE_KEYS answers}}.
    A program dump's first word is the images per BatchNorm group, n / groups; the other 47 words depend on the shape alone, so
    they are kept once per shape (asserted here for every descriptor, so nothing of a dump goes unrecorded).  A descriptor the
    library refuses keeps its (negative) status in place of the dump."""
    lib = cabi._lib
    programs, routes = {}, {}
    for (n, hi, wi, s, p, t, g) in descriptors():
        d = cabi.Conv64Desc(n, hi, wi, out_size(hi, s, p, t), out_size(wi, s, p, t), 3, s, p, t, g)
        ref = ctypes.byref(d)
        dumps = []
        for backward in (0, 1):
            buf = (ctypes.c_int * 64)()
            cnt = lib.srlz_conv64_debug_program(ref, backward, buf, 64)
            if cnt > 0:
                assert buf[0] == n // g, (n, g, buf[0])
            dumps.append(list(buf)[1:cnt] if cnt > 0 else cnt)
        shape = "%dx%d_s%dp%dt%d" % (hi, wi, s, p, t)
        assert programs.setdefault(shape, dumps) == dumps, "the program of %s depends on n = %d, groups = %d" % (shape, n, g)
        routes["n%d_g%d_%s" % (n, g, shape)] = [
            lib.srlz_conv64_fwd_tiles(ref), lib.srlz_conv64_bwd_data_tiles(ref), lib.srlz_conv64_gather_pipe_supported(ref, 0),
            lib.srlz_conv64_gather_pipe_supported(ref, 1), lib.srlz_conv64_bwd_fused_supported(ref),
            lib.srlz_conv64_bwd_fused_bn_rows(ref)]
    return {"programs": programs, "routes": routes}


def test_routes_match_the_recorded_table(cabi):
    assert not os.environ.get("SRLZ_ABLATE"), "the ablation switches change the routes"
    want = json.load(open(GOLDEN))
    got = record(cabi)
    for part in ("programs", "routes"):
        assert sorted(got[part]) == sorted(want[part]), "the descriptor sweep and the fixture differ"
        wrong = {k: (got[part][k], want[part][k]) for k in got[part] if got[part][k] != want[part][k]}
        assert not wrong, "%d of %d %s changed, e.g. %r" % (len(wrong), len(got[part]), part, sorted(wrong.items())[0])
    # the sweep reaches both answers of every predicate
    for i in (2, 3, 4):
        assert {r[i] for r in got["routes"].values()} == {0, 1}, ROUTE_KEYS[i]


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "srl-zoo_amd"))
    from srlz import _cabi
    table = record(_cabi)
    with open(GOLDEN, "w") as f:  # one shape / one descriptor per line
        parts = ['"%s":{\n%s\n}' % (part, ",\n".join('"%s":%s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in sorted(table[part].items())))
                 for part in ("programs", "routes")]
        f.write("{" + ",\n".join(parts) + "}\n")
    print("%d descriptors, %d shapes -> %s" % (len(table["routes"]), len(table["programs"]), GOLDEN))
