"""The plan of a column-partitioned double-precision run (csrc/lbm_plan.cpp plan64_cols, PlanCols64 of lbm_internal.h) through the
lbm_plan64_cols* entry points, without a GPU: which runs are taken and with what storage, tiles and kernel on each rank, field by field
against formulas written here; that every owned cell of a rank has one owning tile and that sub-step 1 stays inside a rank's storage
columns, worked out from the plan's fields alone; K from the knob; the launches of a run; the refusals."""
import ctypes as C

import numpy as np
import pytest

TX, TY, LANES, ACCS = 32, 16, 512, 4
DEFAULT_K = 4
FLAG_NT, FLAG_NO_NT = 1, 2


def multi_ex(e):
    return 2 * ((e + 1) // 2)


def multi64_lds_bytes(k):
    """lbm_geometry.h: the frame's nine planes and a flag byte per cell, the reduction scratch."""
    return (TX + 2 * multi_ex(k - 1)) * (TY + 2 * (k - 1)) * (9 * 8 + 1) + 8 * ACCS * (LANES // 64)


def plane_stride(ncells, skew=24):
    """lbm_plan.cpp plane_stride_floats with the default skew."""
    s = (ncells + 64 + 63) // 64 * 64
    if (s // 64) % 2 == 0:
        s += 64
    if ncells >= 1 << 20:
        s += 64 * skew
    return s


def decompose_columns(nx, nranks):
    """lbm_decompose_columns: whole x-pairs, the spare pairs to the first ranks."""
    pairs, spare = divmod(nx // 2, nranks)
    nxl = [2 * (pairs + (1 if r < spare else 0)) for r in range(nranks)]
    return nxl, [sum(nxl[:r]) for r in range(nranks)]


class PlanCols64(C.Structure):
    """struct PlanCols64 (lbm_internal.h), field for field."""

    _fields_ = [("flags", C.c_uint), ("nranks", C.c_int), ("rank", C.c_int), ("x0", C.c_int), ("nxl", C.c_int), ("pitch", C.c_int),
                ("K", C.c_int), ("ghost", C.c_int), ("n_tiles", C.c_int), ("tiles_x", C.c_int), ("edge", C.c_int), ("nt_stores", C.c_int),
                ("block", C.c_int), ("lds_bytes", C.c_int), ("mask_words", C.c_int), ("partials_cap", C.c_int),
                ("ps", C.c_longlong), ("grid_doubles", C.c_longlong)]


@pytest.fixture(scope="module")
def f64(lbm):
    from mpilattice_boltzmann_amd import f64 as mod
    mod.load_cols_library()
    return mod


@pytest.fixture(scope="module")
def api(lbm, f64):
    lib = lbm.load_library()
    P = C.POINTER
    lib.lbm_plan64_cols_sizeof.restype, lib.lbm_plan64_cols_sizeof.argtypes = C.c_int, []
    lib.lbm_plan64_cols.restype, lib.lbm_plan64_cols.argtypes = C.c_int, [P(f64.CParams64), C.c_int, C.c_int, C.c_uint, P(PlanCols64)]
    lib.lbm_plan64_cols_kernel_name.restype, lib.lbm_plan64_cols_kernel_name.argtypes = C.c_int, [P(PlanCols64), C.c_char_p, C.c_size_t]
    lib.lbm_plan64_cols_run_launches.restype = C.c_int
    lib.lbm_plan64_cols_run_launches.argtypes = [P(PlanCols64), C.c_int, P(C.c_int), P(C.c_int), C.c_int]
    return lib


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in ("LBM_TUNE_MAXBLOCKS", "LBM_TUNE_SKEW", "LBM_TUNE_MULTI64_K", "LBM_TUNE_MULTI64_MIN"):
        monkeypatch.delenv(k, raising=False)


def _plan(api, f64, nx, ny, nranks, rank, flags=0):
    plan, name = PlanCols64(), C.create_string_buffer(128)
    rc = api.lbm_plan64_cols(C.byref(f64.CParams64(nx, ny, 10, 10, 0.1, 0.005, 1.85)), nranks, rank, flags, C.byref(plan))
    if rc == 0:
        assert api.lbm_plan64_cols_kernel_name(C.byref(plan), name, 128) == 0
    return rc, plan, name.value.decode()


def test_layout_mirror(api):
    assert api.lbm_plan64_cols_sizeof() == C.sizeof(PlanCols64) == 16 * 4 + 2 * 8


# (nx, ny, ranks, columns per rank)
SHAPES = [(32, 16, 1, [32]), (64, 16, 2, [32, 32]), (96, 16, 3, [32, 32, 32]), (70, 18, 2, [36, 34]), (8192, 8192, 8, [1024] * 8),
          (65536, 128, 8, [8192] * 8)]


def _expected_name(K, nt, edge):
    return f"lbm_cols_multi_kernel_f64<{K}" + (",nt" if nt else "") + (",edge" if edge else "") + ">"


def _check_rank(c, name, nx, ny, nranks, r, nxl, x0, K, flags=0):
    G = 2 * -(-K // 2)
    pitch = nxl + 2 * G
    storage = pitch * ny
    edge = nxl % TX != 0 or ny % TY != 0
    nt = 2 * 9 * 8 * storage > 192 << 20                                  # plan64_whole's rule on the rank's two grids
    if flags & FLAG_NT:
        nt = True
    if flags & FLAG_NO_NT:
        nt = False
    assert (c.flags, c.nranks, c.rank) == (flags, nranks, r)
    assert (c.x0, c.nxl, c.pitch) == (x0, nxl, pitch) and c.pitch % 2 == 0
    assert (c.K, c.ghost) == (K, G)
    assert (c.tiles_x, c.n_tiles, c.edge) == (-(-nxl // TX), -(-nxl // TX) * -(-ny // TY), int(edge))
    assert c.nt_stores == int(nt) and name == _expected_name(K, nt, edge)
    assert c.block == LANES and c.lds_bytes == multi64_lds_bytes(K) and c.lds_bytes <= 65536
    assert c.mask_words == (storage + 31) // 32 + 4 and c.partials_cap == K * c.n_tiles + 1
    assert c.ps == plane_stride(storage) and c.ps % 2 == 0 and c.ps >= storage + 64 and c.grid_doubles == 9 * c.ps + 128
    assert storage <= 2 ** 31 - 4096


@pytest.mark.parametrize("K", [None, 2, 3, 4, "nonsense"])
@pytest.mark.parametrize("nx,ny,nranks,cols", SHAPES)
def test_plan_field_by_field(lbm, api, f64, monkeypatch, nx, ny, nranks, cols, K):
    if K is not None:
        monkeypatch.setenv("LBM_TUNE_MULTI64_K", str(K))
    K = K if isinstance(K, int) else DEFAULT_K                           # a malformed value: the default
    assert {2: 2, 3: 4, 4: 4}[K] == 2 * -(-K // 2)
    nxl, dis = decompose_columns(nx, nranks)
    got_nxl, got_dis = (C.c_int * nranks)(), (C.c_int * nranks)()
    assert lbm.load_library().lbm_decompose_columns(nx, nranks, got_nxl, got_dis) == 0
    assert nxl == cols and (list(got_nxl), list(got_dis)) == (nxl, dis)
    for r in range(nranks):
        rc, c, name = _plan(api, f64, nx, ny, nranks, r)
        assert rc == 0, lbm.load_library().lbm_last_error()
        _check_rank(c, name, nx, ny, nranks, r, nxl[r], dis[r], K)
    if (nx, ny) == (70, 18):
        a, b = (_plan(api, f64, nx, ny, 2, r)[1] for r in range(2))
        assert (a.pitch, b.pitch) == (36 + 2 * a.ghost, 34 + 2 * a.ghost) and a.edge == b.edge == 1 and a.n_tiles == b.n_tiles == 4


@pytest.mark.parametrize("flags,nt", [(FLAG_NT, True), (FLAG_NO_NT, False)])
def test_store_flags(api, f64, flags, nt):
    rc, c, name = _plan(api, f64, 64, 16, 2, 1, flags)
    assert rc == 0
    _check_rank(c, name, 64, 16, 2, 1, 32, 32, DEFAULT_K, flags)
    rc, c, name = _plan(api, f64, 65536, 128, 8, 3, flags)
    assert rc == 0 and c.nt_stores == int(nt) and name == _expected_name(DEFAULT_K, nt, False)


# (nx, ny, ranks): one rank that is its own neighbour, even ranks, uneven ranks (70: 36 + 34; 198 on 3: 66 + 66 + 66; 200 on 3: 68 + 66
# + 66), a rank that 32 x 16 tiles cover beside one they do not (126 on 2: 64 + 62), a large run
OWNER_CASES = [(32, 16, 1), (34, 18, 1), (64, 16, 2), (70, 18, 2), (126, 32, 2), (198, 50, 3), (200, 33, 3), (8192, 190, 8)]


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("nx,ny,nranks", OWNER_CASES)
def test_ownership_and_bounds_from_the_plan_alone(api, f64, lbm, monkeypatch, nx, ny, nranks, K):
    """Every rank's PlanCols64 from the library, and from ITS fields alone (x0, nxl, pitch, ghost, K, tiles_x, n_tiles, edge, mask_words,
    ps, grid_doubles) what the kernel and the push do with them (kernels/cols64.h): tile (tx, ty) of a rank starts at owned column
    min(TX tx, nxl - TX) and row min(TY ty, ny - TY) and owns its cells at tile-local x >= TX tx - x0, y >= TY ty - y0.
      - every cell of the WHOLE grid has exactly one owning tile of one rank;
      - sub-step 1 of a launch of k <= K steps computes storage columns ghost + x0 - gx .. ghost + x0 + TX + gx - 1, gx = multi_ex(k - 1):
        inside 0 .. pitch - 1, first column even; a cell it must get right (distance <= k - 1) pulls from columns inside the storage; any
        other pulls from column -1 or pitch at the most, which pull_pair_f64's own wrap turns into a cell of the same storage row;
      - the largest storage cell index fits the bitfield and 32 bits, the planes hold the storage and the guards of the shifted loads;
      - a push reads owned columns and writes the NEIGHBOUR's ghost columns, formed from the neighbour's plan: inside its pitch, and
        disjoint from what the neighbour's own push reads, even where a rank is its own neighbour."""
    monkeypatch.setenv("LBM_TUNE_MULTI64_K", str(K))
    plans = []
    for r in range(nranks):
        rc, c, _ = _plan(api, f64, nx, ny, nranks, r)
        assert rc == 0, lbm.load_library().lbm_last_error()
        plans.append(c)
    owners = np.zeros((ny, nx), np.int32)
    at = 0
    for r, c in enumerate(plans):
        assert c.K == K and c.x0 == at and c.pitch == c.nxl + 2 * c.ghost and c.pitch % 2 == 0 and c.ghost % 2 == 0 and c.ghost >= c.K
        at += c.nxl
        assert c.n_tiles % c.tiles_x == 0
        tiles_y = c.n_tiles // c.tiles_x
        assert c.tiles_x * TX >= c.nxl > (c.tiles_x - 1) * TX and tiles_y * TY >= ny > (tiles_y - 1) * TY
        assert c.edge == int(c.tiles_x * TX != c.nxl or tiles_y * TY != ny)
        storage = c.pitch * ny
        assert storage - 1 < 2 ** 31 - 4096 and c.mask_words * 32 >= storage
        assert c.ps >= storage + 64 and c.grid_doubles >= 9 * c.ps + 64      # a shifted load reads one double before or behind a plane's cells
        assert c.partials_cap >= c.K * c.n_tiles
        for ty in range(tiles_y):
            for tx in range(c.tiles_x):
                x0, y0 = min(TX * tx, c.nxl - TX), min(TY * ty, ny - TY)     # the kernel's rule (EDGE; without it the minimum is TX tx)
                if not c.edge:
                    assert (x0, y0) == (TX * tx, TY * ty)
                assert x0 % 2 == 0 and 0 <= x0 <= c.nxl - TX and 0 <= y0 <= ny - TY
                owners[y0 + (TY * ty - y0):y0 + TY, c.x0 + x0 + (TX * tx - x0):c.x0 + x0 + TX] += 1
                for k in range(1, c.K + 1):
                    e = k - 1
                    gx = multi_ex(e)
                    first, last = c.ghost + x0 - gx, c.ghost + x0 + TX + gx - 1       # the storage columns sub-step 1 computes
                    assert 0 <= first and last <= c.pitch - 1 and first % 2 == 0
                    assert 0 <= c.ghost + x0 - e - 1 and c.ghost + x0 + TX + e <= c.pitch - 1   # what a needed cell pulls from
                    assert -1 <= first - 1 and last + 1 <= c.pitch                    # what any computed cell pulls from, before the wrap
                    assert TY > e and ny >= TY                                        # one correction wraps a row
                # the final store: storage columns ghost + x0 .. ghost + x0 + TX - 1 are owned columns
                assert c.ghost <= c.ghost + x0 and c.ghost + x0 + TX - 1 <= c.ghost + c.nxl - 1
        west, east = plans[(r - 1) % nranks], plans[(r + 1) % nranks]
        read = set(range(c.ghost, 2 * c.ghost)) | set(range(c.nxl, c.nxl + c.ghost))                # this rank's push reads these of its own storage
        assert read <= set(range(c.ghost, c.ghost + c.nxl))                                         # owned columns
        into_west = set(range(west.ghost + west.nxl, west.ghost + west.nxl + c.ghost))              # the west rank's east ghost columns
        into_east = set(range(0, c.ghost))                                                          # the east rank's west ghost columns
        assert max(into_west) == west.pitch - 1 and max(into_east) < east.ghost + 1 <= east.pitch
        for other, written in ((west, into_west), (east, into_east)):
            other_reads = set(range(other.ghost, 2 * other.ghost)) | set(range(other.nxl, other.nxl + other.ghost))
            assert not (written & other_reads) and not (written & set(range(other.ghost, other.ghost + other.nxl)))
    assert at == nx and np.all(owners == 1)


@pytest.mark.parametrize("K", [None, 2, 3])
def test_run_launches(api, f64, monkeypatch, K):
    if K is not None:
        monkeypatch.setenv("LBM_TUNE_MULTI64_K", str(K))
    K = DEFAULT_K if K is None else K
    rc, c, _ = _plan(api, f64, 70, 18, 2, 1)
    assert rc == 0 and c.K == K
    for n in (0, 1, K, 37):
        steps, full = (C.c_int * 64)(), (C.c_int * 64)()
        count = api.lbm_plan64_cols_run_launches(C.byref(c), n, steps, full, 64)
        want = [K] * (n // K) + ([n % K] if n % K else [])
        assert count == len(want) == -(-n // K)
        assert list(steps[:count]) == want and list(full[:count]) == [int(k == K) for k in want]
    assert api.lbm_plan64_cols_run_launches(C.byref(c), -1, None, None, 0) == -1
    assert api.lbm_plan64_cols_run_launches(None, 4, None, None, 0) == -1
    assert api.lbm_plan64_cols_run_launches(C.byref(c), 37, None, None, 0) == -(-37 // K)      # cap 0: the count alone


def _message(lbm):
    return lbm.load_library().lbm_last_error().decode()


def test_refusals(lbm, api, f64, digests):
    """Every shape and flag the column partition does not take, each with a message that names the alternative where there is one."""
    from conftest import deck_paths
    p = f64.read_params64(deck_paths("column_24x20", digests)[0])
    assert (p.nx, p.ny) == (24, 20)
    for nx, ny, nranks, text in ((63, 16, 1, "nx must be even"), (62, 16, 2, "leaves rank 1 30 columns"), (p.nx, p.ny, 1, "leaves rank 0 24 columns"),
                                 (64, 15, 2, "ny = 15 is fewer than 16 rows"), (32, 16, 2, "leaves rank 0 16 columns"), (4, 16, 2, "leaves rank 0 2 columns"),
                                 (2, 16, 3, "without an x-pair")):
        assert _plan(api, f64, nx, ny, nranks, 0)[0] == 1
        assert text in _message(lbm) and "row partition" in _message(lbm) and "lbm_rows64_create" in _message(lbm), _message(lbm)
    assert decompose_columns(62, 2)[0] == [32, 30]
    for nranks in (0, 65, -1):
        assert _plan(api, f64, 65 * 64, 16, nranks, 0)[0] == 1 and "nranks must be 1..64" in _message(lbm)
    assert _plan(api, f64, 64 * 64, 16, 64, 63)[0] == 0
    for rank in (-1, 2):
        assert _plan(api, f64, 64, 16, 2, rank)[0] == 1 and "rank outside" in _message(lbm)
    for flags in (512, 1024, 2048, 4096, 8192, 256, 512 | 1, 3 | 4):
        assert _plan(api, f64, 64, 16, 2, 0, flags)[0] == 1
        assert "LBM_FLAG_NT_STORES or LBM_FLAG_NO_NT_STORES only" in _message(lbm)
    assert api.lbm_plan64_cols(C.byref(f64.CParams64(64, 16, 10, 10, 0.1, 0.005, 1.85)), 2, 0, 0, None) == 1
    assert api.lbm_plan64_cols(None, 2, 0, 0, C.byref(PlanCols64())) == 1


def test_a_rank_too_large_for_32_bit_cell_indices_is_refused(lbm, api, f64):
    """The rule of the existing plans, on a RANK's storage: pitch * ny cells must stay below 2^31 - 4096."""
    ny = 1 << 20
    assert (2038 + 8) * ny <= 2 ** 31 - 4096 < (2040 + 8) * ny           # G = 4 at the default K
    assert _plan(api, f64, 2038 * 2, ny, 2, 0)[0] == 0
    assert _plan(api, f64, 2040 * 2, ny, 2, 0)[0] == 1 and "32-bit cell indices" in _message(lbm)
    assert _plan(api, f64, 2040 * 2, ny, 4, 0)[0] == 0                   # the same grid on more ranks
