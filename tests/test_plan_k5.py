"""The plan's side of the five-step launch of whole periodic grids (csrc/lbm_plan.cpp, csrc/lbm_geometry.h), on a CPU: how a run is cut
into launches of 5, 4 and 3 steps, that the cuts of K <= 4 are the parent's, which contexts take lbm_multi_kernel<5> and which keep
what they had, and the LDS a block of it takes."""
import ctypes as C
import json
import os

import pytest

from test_plan import CPlan, GEOM_NARROW, GEOM_STD, GEOM_TALL, no_knobs, plan_of, planner, whole  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE_STEPS_MIN = 1 << 26   # LBM_TUNE_MULTI5_MIN's default, cells: the measured N of DESIGN.md section 4.2 (None: K = 5 is no default anywhere)
ROWS, ROWS5 = 192, 4       # the kernel table: multi_row's rows, then one row per terms index of the five-step launch


@pytest.fixture(scope="module")
def nexts(lbm):
    lib = lbm.load_library()
    lib.lbm_plan_next.restype, lib.lbm_plan_next.argtypes = C.c_int, [C.c_int] * 4
    return lib.lbm_plan_next


def cut(nexts, K, n, four_rows=1, tail4=1):
    out = []
    while n > 0:
        out.append(nexts(K, four_rows, tail4, n))
        assert 1 <= out[-1] <= n
        n -= out[-1]
    return out


def fewest(n):
    """Fewest launches of 5, 4 or 3 steps that add up to n (None: no such split)."""
    best = {0: 0}
    for m in range(1, n + 1):
        c = [best[m - k] for k in (3, 4, 5) if m - k in best and best[m - k] is not None]
        best[m] = min(c) + 1 if c else None
    return best[n]


def test_a_five_step_run_is_cut_into_fives_a_four_and_threes(nexts):
    assert cut(nexts, 5, 11) == [5, 3, 3] and cut(nexts, 5, 12) == [5, 4, 3] and cut(nexts, 5, 6) == [3, 3] and cut(nexts, 5, 7) == [4, 3]
    for n in range(1, 41):
        steps = cut(nexts, 5, n)
        assert sum(steps) == n
        if n < 3:
            assert steps == [n]
        else:
            assert set(steps) <= {5, 4, 3} and len(steps) == fewest(n), (n, steps)
        assert cut(nexts, 5, n, tail4=0) == [5] * (n // 5) + ([n % 5] if n % 5 else [])       # LBM_TUNE_MULTI_TAIL4=0: plain


def test_the_cuts_of_up_to_four_steps_are_the_parents(nexts):
    with open(os.path.join(ROOT, "tests", "golden", "plan_next_parent.json")) as fh:
        table = json.load(fh)["next"]
    assert len(table) == 16
    for key, row in table.items():
        K, four_rows, tail4 = (int(v) for v in key.split(","))
        assert [nexts(K, four_rows, tail4, left) for left in range(1, 41)] == row, key


def five_knobs(env, k="5"):
    env.setenv("LBM_TUNE_MULTI_K", k)


def test_which_contexts_take_the_five_step_launch(lbm, planner, no_knobs):
    big = plan_of(lbm, planner, whole(8192, 8192))
    if FIVE_STEPS_MIN is None:
        assert big[1] == "lbm_multi_kernel<4>" and big[0].multi_K == 4
    else:
        assert big[1] == "lbm_multi_kernel<5>" and (big[0].multi_K, big[0].multi_geom) == (5, GEOM_TALL)
        assert FIVE_STEPS_MIN >= 1 << 22
        side = int(round(FIVE_STEPS_MIN ** 0.5))
        assert side * side == FIVE_STEPS_MIN
        at = plan_of(lbm, planner, whole(side, side))
        assert at[1] == "lbm_multi_kernel<5>" and at[0].partials_cap >= 5 * at[0].multi_tiles_x * ((side + 12) // 13) + 1
        below = plan_of(lbm, planner, whole(side, side - 64))
        assert below[1] == "lbm_multi_kernel<4>" and below[0].multi_K == 4
        for flag in ("FLAG_EXACT_AVVELS", "FLAG_FAST_AVVELS", "FLAG_FUSED_ARITH"):
            assert plan_of(lbm, planner, whole(8192, 8192, flag))[0].multi_K == 5
    # whatever the default: partitions, tile ranks and the other geometries keep four steps per launch at any size
    ring = plan_of(lbm, planner, {"kind": "ring", "nx": 8192, "ny": 8192, "flags": ["FLAG_FORCE_HALO"], "env": {}})
    assert ring[0].multi_K == 4 and ring[0].ghost > 0
    tile = plan_of(lbm, planner, {"kind": "tile", "nx": 8192, "ny": 8192, "px": 2, "py": 2, "rank": 3, "flags": [], "env": {}})
    assert tile[0].multi_K == 4 and tile[0].ghost_x > 0
    no_knobs.setenv("LBM_TUNE_MULTI_GEOM", str(GEOM_STD))
    assert plan_of(lbm, planner, whole(8192, 8192))[1] == "lbm_multi_kernel<4>"
    no_knobs.setenv("LBM_TUNE_MULTI_GEOM", str(GEOM_NARROW))
    assert plan_of(lbm, planner, whole(8192, 8192))[1] == "lbm_multi_kernel<4>"
    no_knobs.delenv("LBM_TUNE_MULTI_GEOM")
    assert plan_of(lbm, planner, whole(1024, 1024))[1] == "lbm_multi_kernel<4>"                 # tests/test_plan.py pins it too
    odd = plan_of(lbm, planner, whole(8191, 8192))                                               # nx the kernel does not tile at all
    assert odd[1].startswith("lbm_step_kernel")


def test_the_knob_selects_five_steps_where_they_are_built(lbm, planner, no_knobs):
    five_knobs(no_knobs)
    no_knobs.setenv("LBM_TUNE_TILE_MAX", "0")
    no_knobs.setenv("LBM_TUNE_MULTI_GEOM", str(GEOM_TALL))
    plan, name = plan_of(lbm, planner, whole(256, 83))
    assert (name, plan.multi_K, plan.multi_geom, plan.multi_tx, plan.multi_tiles_x) == ("lbm_multi_kernel<5>", 5, GEOM_TALL, 64, 4)
    assert plan.partials_cap >= 5 * 4 * 7 + 1                          # five vectors over the tiles of its shortest tail (13-row tiles)
    for flag, words in (("FLAG_EXACT_AVVELS", "lbm_multi_kernel<5, double-precision av_vels terms>"), ("FLAG_FAST_AVVELS", "lbm_multi_kernel<5, fast av_vels>"),
                        ("FLAG_FUSED_ARITH", "lbm_multi_kernel<5, 6> (fused arithmetic)")):
        assert plan_of(lbm, planner, whole(256, 83, flag))[1] == words
    no_knobs.delenv("LBM_TUNE_MULTI_GEOM")
    assert plan_of(lbm, planner, whole(1024, 1024))[1] == "lbm_multi_kernel<5>"                 # tall by size
    # not eligible: the clamp to four steps, as for any value above the largest built
    assert plan_of(lbm, planner, whole(768, 768))[1] == "lbm_multi_kernel<4>"                   # standard geometry by size
    no_knobs.setenv("LBM_TUNE_MULTI_GEOM", str(GEOM_NARROW))
    assert plan_of(lbm, planner, whole(1024, 1024))[1] == "lbm_multi_kernel<4>"
    no_knobs.delenv("LBM_TUNE_MULTI_GEOM")
    no_knobs.setenv("LBM_TUNE_MACRO_K", "5")
    ring = plan_of(lbm, planner, {"kind": "ring", "nx": 1024, "ny": 1024, "flags": ["FLAG_FORCE_HALO"], "env": {}})
    assert ring[0].multi_K == 4
    tile = plan_of(lbm, planner, {"kind": "tile", "nx": 2048, "ny": 2048, "px": 2, "py": 1, "rank": 0, "flags": [], "env": {}})
    assert tile[0].multi_K == 4
    five_knobs(no_knobs, "9")
    assert plan_of(lbm, planner, whole(1024, 1024))[1] == "lbm_multi_kernel<5>" and plan_of(lbm, planner, whole(768, 768))[1] == "lbm_multi_kernel<4>"


def test_the_threshold_knob(lbm, planner, no_knobs):
    no_knobs.setenv("LBM_TUNE_MULTI5_MIN", str(1 << 20))
    assert plan_of(lbm, planner, whole(1024, 1024))[1] == "lbm_multi_kernel<5>"
    assert plan_of(lbm, planner, whole(1024, 960))[1] == "lbm_multi_kernel<4>"
    no_knobs.setenv("LBM_TUNE_MULTI5_MIN", "0")
    assert plan_of(lbm, planner, whole(8192, 8192))[1] == "lbm_multi_kernel<4>"


def test_launches_of_a_five_step_context(lbm, planner, no_knobs):
    """Every launch of a 12-step run: 5 + 4 + 3, each on its own geometry and table row; the rows of the existing table do not move."""
    import test_launch_plan as tl
    five_knobs(no_knobs)
    plan, _ = plan_of(lbm, planner, whole(1024, 1024))
    lib = planner
    lib.lbm_plan_run_launches.restype, lib.lbm_plan_run_launches.argtypes = C.c_int, [C.POINTER(CPlan), C.c_int, C.c_int, C.POINTER(tl.CLaunch), C.c_int]
    lib.lbm_plan_launch_sizeof.restype, lib.lbm_plan_launch_sizeof.argtypes = C.c_int, []
    assert lib.lbm_plan_launch_sizeof() == C.sizeof(tl.CLaunch)
    out = (tl.CLaunch * 8)()
    assert lib.lbm_plan_run_launches(C.byref(plan), 12, 0, out, 8) == 3
    five, four, three = out[0], out[1], out[2]
    assert (five.k, five.row, five.lanes, five.part, five.ntiles_total) == (5, ROWS + 2, 768, 0, 16 * 43)          # terms index 2: compensated
    assert (four.k, four.lanes, four.ntiles_total) == (4, 768, 16 * 43) and four.row < ROWS and (four.row % 4, four.row // 4 % 4, four.row // 16 % 4 + 1, four.row // 64) == (0, 2, 4, GEOM_TALL)
    assert (three.k, three.lanes, three.ntiles_total) == (3, 512, 16 * 64) and (three.row // 16 % 4 + 1, three.row // 64) == (3, GEOM_TALL)
    assert max(l.k * l.ntiles_total for l in (five, four, three)) + 1 <= plan.partials_cap


def test_lds_of_the_five_step_launch(lbm):
    lib = lbm.load_library()
    lib.lbm_plan_multi_lds_bytes.restype, lib.lbm_plan_multi_lds_bytes.argtypes = C.c_int, [C.c_int, C.c_int]
    five = lib.lbm_plan_multi_lds_bytes(5, GEOM_TALL)
    assert five == 8 * 72 * 32 * 4 + 384 * 8 + 72 * 32 // 2 + 5 * 12 * 8 == 78432 <= 80 * 1024
    assert lib.lbm_plan_multi_lds_bytes(4, GEOM_TALL) == 9 * 72 * 30 * 4 + 72 * 30 // 2 + 4 * 12 * 8                  # the parent's formula
    assert lib.lbm_plan_multi_lds_bytes(3, GEOM_TALL) == lib.lbm_plan_multi_lds_bytes(3, GEOM_STD) == 9 * 68 * 20 * 4 + 68 * 20 // 2 + 3 * 8 * 8
    assert lib.lbm_plan_multi_lds_bytes(5, GEOM_STD) == -1 and lib.lbm_plan_multi_lds_bytes(5, GEOM_NARROW) == -1     # not built
