"""The weight-gradient plan of the 64->64 convolution family (srlz_conv64_bwd_weight_plan: the host-only answer computed by the code
srlz_conv64_bwd_weight launches from, csrc/conv64_wgrad.hip), over the descriptor sweep of test_conv64_routes_cpu.py crossed with a
fused x_bnp and a gradient rebuilt from (dA, y).  Host code only: no GPU.

The ROUTE (which of the four kernels runs) depends on the shape and the operands alone and is pinned in
tests/golden/conv64_wgrad_routes.json.  The grid and the chunks per workgroup follow the device's CU count, so they are held to
invariants instead.  To record the routes again (only when a route is meant to change):  python tests/test_conv64_wgrad_plan_cpu.py
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_conv64_routes_cpu import descriptors, out_size  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "conv64_wgrad_routes.json")
ROUTES = ("ring_s2", "ring", "gather", "chunk")
PARTIAL_BYTES = (9 * 64 * 64 + 64) * 4  # one workgroup's partial: nine taps of 64 x 64 and the bias sums (include/srlz.h: split-K partials)
OPERANDS = ((0, 0), (1, 0), (0, 1), (1, 1))  # (has_x_bnp, has_dy_bn)


def plans(cabi):
    """(key, descriptor tuple, has_x_bnp, has_dy_bn, [route, workgroups, cpw, tk] or the negative status of a refused descriptor)"""
    lib = cabi._lib
    for (n, hi, wi, s, p, t, g) in descriptors():
        d = cabi.Conv64Desc(n, hi, wi, out_size(hi, s, p, t), out_size(wi, s, p, t), 3, s, p, t, g)
        for (xb, db) in OPERANDS:
            out = (ctypes.c_int * 4)(-1, -1, -1, -1)
            rc = lib.srlz_conv64_bwd_weight_plan(ctypes.byref(d), xb, db, out)
            yield "n%d_g%d_%dx%d_s%dp%dt%d_x%d_d%d" % (n, g, hi, wi, s, p, t, xb, db), d, xb, db, (list(out) if rc == 0 else rc)


def record(cabi):
    return {k: (pl[0] if isinstance(pl, list) else pl) for k, _, _, _, pl in plans(cabi)}


def test_routes_match_the_recorded_table(cabi):
    assert not os.environ.get("SRLZ_ABLATE"), "the ablation switches change the routes"
    want = json.load(open(GOLDEN))
    got = record(cabi)
    assert sorted(got) == sorted(want), "the descriptor sweep and the fixture differ"
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, "%d of %d routes changed, e.g. %r" % (len(wrong), len(got), sorted(wrong.items())[0])
    assert {r for r in got.values() if r >= 0} == {0, 1, 2, 3}, "the sweep reaches all four routes"


def test_operands_move_the_route_only_towards_the_chunk_kernel(cabi):
    """A gradient rebuilt from (dA, y) is staged by conv64_wgrad_kernel alone; the gather kernel has no fused x_bnp; both ring kernels
    take one."""
    got = record(cabi)
    for k, r in got.items():
        if not k.endswith("_x0_d0") or r < 0:
            continue
        base = k[:-len("_x0_d0")]
        assert got[base + "_x0_d1"] == 3 and got[base + "_x1_d1"] == 3, k
        assert got[base + "_x1_d0"] == (3 if r == 2 else r), k


def test_grid_and_chunks_per_workgroup_invariants(cabi):
    lib = cabi._lib
    cus = cabi.device_cus()
    seen = set()
    for key, d, xb, db, pl in plans(cabi):
        ws = lib.srlz_conv64_bwd_weight_workspace(ctypes.byref(d))
        if not isinstance(pl, list):
            assert ws == 0, key
            continue
        route, wgs, cpw, tk = pl
        G = max(d.groups, 1)
        prog = (ctypes.c_int * 64)()
        assert lib.srlz_conv64_debug_program(ctypes.byref(d), 0, prog, 64) > 0
        total_q = prog[0] * prog[1] * prog[2]  # grid positions per BatchNorm group: images x PH x PW
        assert tk == (32 if route == 0 else 64), key
        nch = (total_q + tk - 1) // tk
        assert wgs >= G and wgs % G == 0 and wgs <= 2 * cus and cpw >= 1, (key, pl)
        # the workspace holds one partial per workgroup of the FULL grid (what the plan may shrink from), whatever the route
        assert ws % PARTIAL_BYTES == 0, key
        grid = ws // PARTIAL_BYTES
        assert grid % G == 0 and wgs <= grid <= 2 * cus, (key, pl, grid)
        wpg, gpg = wgs // G, grid // G
        if route in (0, 1):  # contiguous ranges of cpw chunks, group by group; the last workgroup of a group takes what is left
            assert cpw == (nch + gpg - 1) // gpg, (key, pl, nch, gpg)
            assert wpg * cpw >= nch > (wpg - 1) * cpw, (key, pl, nch)
        else:  # all groups' chunks strided over the whole grid
            assert wgs == grid, (key, pl, grid)
            assert wgs * cpw >= nch * G > wgs * (cpw - 1), (key, pl, nch)
        seen.add((route, min(cpw, 2)))
    # every route both with one chunk per workgroup and in its steady state
    assert seen == {(r, c) for r in range(4) for c in (1, 2)}, sorted(seen)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "srl-zoo_amd"))
    from srlz import _cabi
    table = record(_cabi)
    with open(GOLDEN, "w") as f:  # one descriptor per line
        f.write("{\n" + ",\n".join('"%s":%d' % kv for kv in sorted(table.items())) + "\n}\n")
    print("%d plans -> %s, routes %s" % (len(table), GOLDEN, sorted(set(table.values()))))
