"""GPU suite of the read-out entry points: lbm_state_checksum, lbm_av_velocity_sum, lbm_get_observables and the lbm_get_cells /
lbm_set_cells pair, each held to a host restatement (tests/readout_ref.py, itself pinned by tests/test_readout_ref.py) of the array
that was put on, or fetched from, the device — at every storage layout the library has: whole grids (wide and narrow kernels' storage,
and one past the first pass of both capped launches), row blocks, K-step partitions with ghost rows, tile ranks with ghost columns, and
a window whose global cell indices need more than 32 bits.

Bars: digests are integers and compared with ==; cells and observables are compared as uint32 bit patterns; the velocity sum is
compared with the exactly rounded sum of the same terms at the bound its summation order allows (readout_ref.velocity_sum_bound),
computed from the number of cells."""
import itertools

import numpy as np
import pytest

import readout_ref
from conftest import deck_paths

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def load_case(lbm, digests, name):
    ppath, opath = deck_paths(name, digests)
    p = lbm.read_params(ppath)
    obst, free = lbm.read_obstacles(opath, p.nx, p.ny)
    return p, obst, free


def random_state(rows, ncol, seed):
    """Ordinary populations (positive, of the size a run has them), so that velocities and observables are ordinary numbers too."""
    rng = np.random.default_rng(seed)
    return (rng.random((rows, ncol, 9), dtype=np.float32) * np.float32(0.02) + np.float32(0.004)).astype(np.float32)


def row_ranges(y0, rows):
    """Global row ranges of a partition of `rows` rows from y0: the first and the last row alone, one row inside, ranges that start / end
    on and off the partition's edges — and empty ones, whose digest is 0."""
    mid = rows // 2
    some = {(0, 1), (rows - 1, rows), (mid, mid + 1), (0, rows // 3), (rows // 3, rows), (1, rows - 1), (mid - 1, min(rows, mid + 6))}
    empty = {(0, 0), (mid, mid), (rows, rows)}
    return sorted((y0 + a, y0 + b) for a, b in some if a < b), sorted((y0 + a, y0 + b) for a, b in empty)


def check_readout(part, cells, obst_block, nx_global, x0=0, fetched=False):
    """`part` holds `cells` — its (ny_local, nx_local, 9) block, first cell at column x0 of global row part.y0 in a grid nx_global wide:
    everything it reports about them against the restatements.  fetched: `cells` came from get_cells (after a run); otherwise they were
    written with set_cells and get_cells must return their bits."""
    rows, ncol, _ = cells.shape
    assert (rows, ncol) == (part.ny_local, part.nx_local) and obst_block.shape == (rows, ncol)
    if not fetched:
        assert np.array_equal(bits(part.get_cells()), bits(cells)), "get_cells does not return what set_cells was given"
    cell0 = part.y0 * nx_global + x0
    want = readout_ref.digest(cells, cell0, nx_global)
    got = part.checksum()
    print(f"digest {got:#018x} (restatement {want:#018x}) rows {rows} cols {ncol} first cell {cell0}")
    assert got == want
    ranges, empty = row_ranges(part.y0, rows)
    for a, b in ranges:
        assert part.checksum(a, b) == readout_ref.digest(cells[a - part.y0:b - part.y0], a * nx_global + x0, nx_global), (a, b)
    for a, b in empty:
        assert part.checksum(a, b) == 0, (a, b)
    # velocity sum: exactly rounded reference, so the whole error is the device's summation order
    exact = readout_ref.velocity_sum(cells, obst_block)
    dev = part.av_velocity_sum()
    bound = readout_ref.velocity_sum_bound(rows * ncol)
    print(f"velocity sum {dev!r} (exactly rounded {exact!r}): relative error {abs(dev - exact) / exact:.3e}, bound {bound:.3e}")
    assert exact > 0 and abs(dev - exact) <= bound * exact
    obs = part.get_observables()
    assert obs.shape == (rows, ncol, 4)
    assert np.array_equal(bits(obs), bits(readout_ref.observables(cells)))


def whole_grid(lbm, nx, ny, seed, density=0.05):
    p = lbm.Params(nx, ny, 10, 4, 0.1, 0.01, 1.7)
    obst = lbm.synthetic_obstacles(nx, ny, density, seed, False)
    return p, obst, lbm.count_free_cells(obst)


# ---- layouts ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", [(64, 48),            # 4 cells per lane
                                   (257, 33),           # odd nx: the one-cell-per-lane kernel's storage
                                   (1536, 1024)])       # 1 572 864 cells: past the first pass of the digest's 4096 x 256 lanes and of the
def test_whole_grid_context(lbm, nx, ny):              # velocity sum's 1024 x 256 (the rest is reached by their stride loops only)
    p, obst, free = whole_grid(lbm, nx, ny, seed=nx + ny)
    cells = random_state(ny, nx, seed=ny)
    with lbm.Partition(p, free, obst) as part:
        part.set_cells(cells)
        check_readout(part, cells, obst, nx)


def test_row_block_with_an_offset(lbm):
    """lbm_create of rows [37, 57) of 80: the digest's global index starts at y0 * nx."""
    nx, ny, y0, rows = 96, 80, 37, 20
    p, obst, free = whole_grid(lbm, nx, ny, seed=5)
    cells = random_state(rows, nx, seed=6)
    with lbm.Partition(p, free, obst[y0:y0 + rows], y0) as part:
        assert part.macro_steps == 0
        part.set_cells(cells)
        check_readout(part, cells, obst[y0:y0 + rows], nx)
        # the same bits in other rows of the grid digest differently
        with lbm.Partition(p, free, obst[y0 + 1:y0 + 1 + rows], y0 + 1) as other:
            other.set_cells(cells)
            assert other.checksum() == readout_ref.digest(cells, (y0 + 1) * nx, nx) != part.checksum()


def test_k_step_partition_with_unaligned_ghost_rows(lbm, monkeypatch):
    """nx = 130, K = 3: the owned rows start ghost * 130 cells into the storage and the obstacle bitfield, not at a multiple of 32 bits."""
    monkeypatch.setenv("LBM_TUNE_MACRO_K", "3")
    nx, ny = 130, 40
    p = lbm.Params(nx, ny, 30, 4, 0.1, 0.01, 1.7)
    obst = lbm.synthetic_obstacles(nx, ny, 0.2, 17, False)
    sim = lbm.Simulation(p, obst, flags=lbm._capi.FLAG_FORCE_HALO, exchange="p2p", strict=True)
    try:
        ghost = sim.partition.tile_info()["ghost"]
        assert sim.partition.macro_steps == 3 and ghost > 0 and (ghost * nx) % 32 != 0
        cells = random_state(ny, nx, seed=8)
        sim.partition.set_cells(cells)
        check_readout(sim.partition, cells, obst, nx)
    finally:
        sim.close()


@pytest.mark.parametrize("rank", [0, 1, 2])
def test_k_step_partition_from_a_rank_window(lbm, rank):
    """lbm_create_rank: ghost rows around the owned rows AND a row offset (ranks 1, 2)."""
    nx, ny, size = 256, 200, 3
    p = lbm.Params(nx, ny, 25, 4, 0.1, 0.01, 1.7)
    obst = lbm.synthetic_obstacles(nx, ny, 0.05, 77, True)
    lay = lbm.rank_layout(p, size, rank)
    ys = slice(lay["y0"], lay["y0"] + lay["ny_local"])
    cells = random_state(lay["ny_local"], nx, seed=20 + rank)
    with lbm.Partition(p, lbm.count_free_cells(obst), lbm.obstacle_window(obst, lay), rank_of=(rank, size)) as part:
        assert part.macro_steps >= 2 and lay["ghost"] > 0 and part.y0 == lay["y0"]
        part.set_cells(cells)
        check_readout(part, cells, obst[ys], nx)


@pytest.mark.parametrize("rank", [0, 1, 2, 3])
def test_every_rank_of_a_tile_decomposition(lbm, rank):
    """2 x 2 ranks of 512 x 256: ghost columns inside the storage rows, x0 > 0 on ranks 1 and 3, y0 > 0 on 2 and 3.  Each rank's digest
    is the restatement's of its own block at its own place in the grid — not merely a term of a sum that comes out right."""
    nx, ny = 512, 256
    p = lbm.Params(nx, ny, 10, 4, 0.1, 0.01, 1.7)
    obst = lbm.synthetic_obstacles(nx, ny, 0.03, 3, False)
    lay = lbm.tile_layout(p, 2, 2, rank)
    ys, xs = slice(lay["y0"], lay["y0"] + lay["ny_local"]), slice(lay["x0"], lay["x0"] + lay["nx_local"])
    assert (lay["x0"] > 0) == (rank in (1, 3)) and (lay["y0"] > 0) == (rank in (2, 3)) and lay["ghost_x"] > 0
    state = random_state(ny, nx, seed=5)
    cells = np.ascontiguousarray(state[ys, xs])
    with lbm.Partition(p, lbm.count_free_cells(obst), lbm.obstacle_window(obst, lay), tile_of=(rank, 2, 2)) as part:
        part.set_cells(cells)
        check_readout(part, cells, obst[ys, xs], nx, x0=lay["x0"])


def test_window_far_into_a_huge_grid(lbm):
    """The last 16 rows of an 8192 x 2^20 grid through lbm_create (which sizes everything by the partition): global cell indices up to
    2^33, index * 9 + k past 2^36 — a 32-bit product anywhere in the digest's index arithmetic shows here."""
    nx, ny, rows = 8192, 2 ** 20, 16
    y0 = ny - rows
    p = lbm.Params(nx, ny, 10, 4, 0.1, 0.01, 1.7)
    obst = lbm.synthetic_obstacles(nx, rows, 0.05, 31, False)
    cells = random_state(rows, nx, seed=32)
    assert (y0 * nx) * 9 > 2 ** 36
    with lbm.Partition(p, 2 ** 31 - 1, obst, y0) as part:       # (free_cells is the global count, an int: it only scales av_vels)
        part.set_cells(cells)
        check_readout(part, cells, obst, nx)
        assert part.checksum() != readout_ref.digest(cells, (y0 * nx) % 2 ** 32, nx)          # what 32-bit indices would give


def test_grid_whose_observables_take_several_launches_by_default(lbm):
    """4100 x 4096 = 16 793 600 cells, above the 16 M cells lbm_get_observables computes per launch: the second launch's row offset;
    16 passes of the digest's stride loop, 64 of the velocity sum's."""
    nx, ny = 4100, 4096
    p, obst, free = whole_grid(lbm, nx, ny, seed=9, density=0.01)
    assert nx * ny > 16 << 20
    cells = random_state(ny, nx, seed=10)
    with lbm.Partition(p, free, obst) as part:
        part.set_cells(cells)
        assert part.checksum() == readout_ref.digest_rows(cells, chunk_rows=256)
        last = ny - 3
        assert part.checksum(last, ny) == readout_ref.digest(cells[last:], last * nx, nx)
        exact = readout_ref.velocity_sum(cells, obst)
        dev = part.av_velocity_sum()
        print(f"velocity sum relative error {abs(dev - exact) / exact:.3e}, bound {readout_ref.velocity_sum_bound(nx * ny):.3e}")
        assert abs(dev - exact) <= readout_ref.velocity_sum_bound(nx * ny) * exact
        obs = part.get_observables()
    for r in range(0, ny, 512):
        assert np.array_equal(bits(obs[r:r + 512]), bits(readout_ref.observables(cells[r:r + 512]))), r


@pytest.mark.parametrize("layout", ["whole", "k_step", "tile"])
def test_observables_fetched_in_row_chunks(lbm, monkeypatch, layout):
    """LBM_TUNE_OBS_CHUNK_CELLS below the partition's size: every launch after the first starts at a row offset — on top of the ghost-row
    offset of a K-step partition, inside the column window of a tile rank."""
    nx, ny = 512, 256
    p = lbm.Params(nx, ny, 10, 4, 0.1, 0.01, 1.7)
    obst = lbm.synthetic_obstacles(nx, ny, 0.03, 3, False)
    free = lbm.count_free_cells(obst)
    state = random_state(ny, nx, seed=12)
    monkeypatch.setenv("LBM_TUNE_OBS_CHUNK_CELLS", str(37 * 256 + 5))          # 18 rows per launch of 512, 37 of 256: neither divides the rows
    if layout == "whole":
        part, cells = lbm.Partition(p, free, obst), state
    elif layout == "k_step":
        lay = lbm.rank_layout(p, 2, 1)
        part = lbm.Partition(p, free, lbm.obstacle_window(obst, lay), rank_of=(1, 2))
        assert part.macro_steps >= 2 and lay["y0"] > 0
        cells = np.ascontiguousarray(state[lay["y0"]:lay["y0"] + lay["ny_local"]])
    else:
        lay = lbm.tile_layout(p, 2, 2, 3)
        part = lbm.Partition(p, free, lbm.obstacle_window(obst, lay), tile_of=(3, 2, 2))
        cells = np.ascontiguousarray(state[lay["y0"]:lay["y0"] + lay["ny_local"], lay["x0"]:lay["x0"] + lay["nx_local"]])
    with part:
        part.set_cells(cells)
        assert np.array_equal(bits(part.get_observables()), bits(readout_ref.observables(cells)))


# ---- sensitivity on the device ----------------------------------------------------------------------------------------------

BIG_NX, BIG_NY = 1536, 1024
FIRST_STRIDE_CELL = 4096 * 256                  # the first cell no lane of the digest's launch reaches without its stride loop
FLIP_CELLS = (0, BIG_NX * BIG_NY - 1, FIRST_STRIDE_CELL, 777 * BIG_NX + 1001)
FLIP_PLANES, FLIP_BITS = (0, 4, 8), (0, 23, 31)        # lowest mantissa bit, lowest exponent bit, sign
# (cell, plane, bit): every cell with every bit, the plane rotating so that every cell meets every plane and every plane every bit — 12 states
# instead of the 36 of the full product (each is a 57 MB set_cells and a host digest of 1.5 M cells: 4.6 s for the 36, a third of this file)
FLIPS = [(cell, FLIP_PLANES[(i + j) % 3], bit) for i, cell in enumerate(FLIP_CELLS) for j, bit in enumerate(FLIP_BITS)]


def test_digest_changes_with_single_bits_and_swaps(lbm):
    """One bit of one population flipped, anywhere in the grid and in the word: the device's digest moves, to the restatement's value of
    the flipped state.  Two neighbouring cells swapped: likewise."""
    nx, ny = BIG_NX, BIG_NY
    assert FIRST_STRIDE_CELL < nx * ny
    assert {(c, k) for c, k, _ in FLIPS} == set(itertools.product(FLIP_CELLS, FLIP_PLANES))
    assert {(k, b) for _, k, b in FLIPS} == set(itertools.product(FLIP_PLANES, FLIP_BITS))
    assert {(c, b) for c, _, b in FLIPS} == set(itertools.product(FLIP_CELLS, FLIP_BITS))
    p, obst, free = whole_grid(lbm, nx, ny, seed=1)
    cells = random_state(ny, nx, seed=2)
    flat = cells.reshape(nx * ny, 9)                          # a view: writes go to `cells`
    with lbm.Partition(p, free, obst) as part:
        part.set_cells(cells)
        base = part.checksum()
        assert base == readout_ref.digest(cells)
        seen = {base}
        for cell, plane, bit in FLIPS:
            flat.view(np.uint32)[cell, plane] ^= np.uint32(1 << bit)
            part.set_cells(cells)
            got = part.checksum()
            assert got != base, (cell, plane, bit)
            assert got == readout_ref.digest(cells), (cell, plane, bit)
            seen.add(got)
            flat.view(np.uint32)[cell, plane] ^= np.uint32(1 << bit)
        assert len(seen) == 1 + len(FLIPS)
        for cell in (0, FIRST_STRIDE_CELL - 1, nx * ny - 2):              # (the middle pair straddles the first pass's end)
            swapped = cells.copy()
            sflat = swapped.reshape(nx * ny, 9)
            sflat[[cell, cell + 1]] = flat[[cell + 1, cell]]
            assert not np.array_equal(bits(swapped), bits(cells))
            part.set_cells(swapped)
            got = part.checksum()
            assert got != base and got == readout_ref.digest(swapped), cell
            assert got not in seen
        part.set_cells(cells)
        assert part.checksum() == base


# ---- values that are not ordinary numbers -----------------------------------------------------------------------------------

SPECIAL_BITS = (0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFFFFFFF, 0x7FFFFFFF,      # quiet NaNs: default, generated, with payload, all ones
                0x7F800001, 0xFF800001, 0x7FA00000, 0x7F812345,                  # signalling NaNs
                0x7F800000, 0xFF800000,                                          # both infinities
                0x80000000, 0x00000000,                                          # -0.0, +0.0
                0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000)      # denormals


def test_cells_and_digest_move_bits_not_numbers(lbm):
    """NaN payloads (quiet and signalling), infinities, -0.0 and denormals go in and come out bit for bit (no flush, no quieting), and the
    digest is the restatement's.  The state is not stepped."""
    nx, ny = 64, 48
    p, obst, free = whole_grid(lbm, nx, ny, seed=4)
    cells = random_state(ny, nx, seed=3)
    raw = cells.view(np.uint32).reshape(-1)
    rng = np.random.default_rng(7)
    where = rng.choice(raw.size, size=40 * len(SPECIAL_BITS), replace=False)
    raw[where] = np.tile(np.array(SPECIAL_BITS, np.uint32), 40)
    raw[:9] = np.array(SPECIAL_BITS[:9], np.uint32)                  # the first cell: nine kinds of NaN
    raw[-9:] = np.array(SPECIAL_BITS[-9:], np.uint32)                # the last: infinities, zeros, denormals
    with lbm.Partition(p, free, obst) as part:
        part.set_cells(cells)
        assert np.array_equal(bits(part.get_cells()), bits(cells))
        assert part.checksum() == readout_ref.digest(cells)
        assert part.checksum(0, 1) == readout_ref.digest(cells[:1]) and part.checksum(ny - 1, ny) == readout_ref.digest(cells[-1:], (ny - 1) * nx, nx)
        # -0.0 for +0.0 in one population is another state
        minus = cells.copy()
        at = np.flatnonzero(raw == 0)[0]
        minus.view(np.uint32).reshape(-1)[at] = 0x80000000
        part.set_cells(minus)
        assert part.checksum() == readout_ref.digest(minus) != readout_ref.digest(cells)
    # a tile rank's column window moves the same bits
    q = lbm.Params(512, 256, 10, 4, 0.1, 0.01, 1.7)
    o = lbm.synthetic_obstacles(512, 256, 0.03, 3, False)
    lay = lbm.tile_layout(q, 2, 2, 3)
    block = random_state(lay["ny_local"], lay["nx_local"], seed=13)
    braw = block.view(np.uint32).reshape(-1)
    braw[rng.choice(braw.size, size=40 * len(SPECIAL_BITS), replace=False)] = np.tile(np.array(SPECIAL_BITS, np.uint32), 40)
    with lbm.Partition(q, lbm.count_free_cells(o), lbm.obstacle_window(o, lay), tile_of=(3, 2, 2)) as part:
        part.set_cells(block)
        assert np.array_equal(bits(part.get_cells()), bits(block))
        assert part.checksum() == readout_ref.digest(block, lay["y0"] * 512 + lay["x0"], 512)


# ---- after real runs --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,steps", [("rand_64x48", 37), ("256x256_t1000", 37), ("1024x1024_t200", 37), ("1024x1024_t200", 8)])
def test_readout_of_a_stepped_grid(lbm, oracle, digests, name, steps):
    """The library's own kernel choice for the deck; an odd and an even number of launches behind the state (which of the two grids is
    current).  The fetched cells are the oracle's; digest, velocity sum and observables are the restatement's of them."""
    p, obst, free = load_case(lbm, digests, name)
    sim = lbm.Simulation(p, obst)
    try:
        sim.run(steps)
        cells = sim.local_cells()
        ref_cells, _, _ = oracle.run(p, obst, steps, nthreads=4)
        assert np.array_equal(bits(cells), bits(ref_cells))
        check_readout(sim.partition, cells, obst, p.nx, fetched=True)
    finally:
        sim.close()


def test_readout_of_a_stepped_one_rank_ring(lbm, oracle, digests):
    """A K-step partition after a run of the peer-to-peer loop: ghost rows around the owned ones, the current grid wherever the groups
    of launches left it."""
    p, obst, free = load_case(lbm, digests, "synth_512x512_t100")
    sim = lbm.Simulation(p, obst, flags=lbm._capi.FLAG_FORCE_HALO, exchange="p2p", strict=True)
    try:
        assert sim.loop == "p2p" and sim.partition.macro_steps >= 2
        sim.run(37)
        cells = sim.local_cells()
        ref_cells, _, _ = oracle.run(p, obst, 37, nthreads=4)
        assert np.array_equal(bits(cells), bits(ref_cells))
        check_readout(sim.partition, cells, obst, p.nx, fetched=True)
    finally:
        sim.close()
