"""The state digest of the double-precision mode, host half (include/lbm_d2q9_f64_digest.h; lbm_digest64_host of csrc/lbm_host.cpp):
the known answers of the definition, the numpy restatement tests/digest64_ref.py on states full of edge values, additivity over row
ranges, sensitivity to one bit and to position, the header as C99, the exports, and every refusal that needs no GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import digest64_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = ref.MASK


@pytest.fixture(scope="module")
def f64(lbm):
    from mpilattice_boltzmann_amd import f64 as mod
    mod.load_digest_library()
    return mod


# ---- the known answers: from a restatement of the definition that is neither the library's nor this file's ---------------------------
SIX_CELLS = (1.0 + np.arange(54)) / 8.0          # 2 rows x 3 columns: AoS value number i is (1 + i) / 8.0


def _both(f64, cells, nx, y0):
    """The library's and the restatement's row digests, which must agree; returns them as Python ints."""
    rows, total = f64.digest_host(cells, nx, y0)
    mine = ref.row_digests(cells, nx, y0)
    assert rows.dtype == np.uint64 and np.array_equal(rows, mine), (rows, mine)
    assert total == sum(int(v) for v in rows) & MASK == ref.digest(cells, nx, y0)
    return [int(v) for v in rows], total


def test_known_answers_six_cells(f64):
    rows, total = _both(f64, SIX_CELLS, 3, 0)
    assert rows == [0xa96575fd2aa0b840, 0x1b8c04ebd0b8b65a] and total == 0xc4f17ae8fb596e9a
    rows, total = _both(f64, SIX_CELLS, 3, 5)
    assert rows == [0x3d372f979e5dd85a, 0x36adf4c564caeb7d] and total == 0x73e5245d0328c3d7


def test_known_answer_cell_indices_beyond_2_to_the_32(f64):
    """One row of 70000 cells that is row 70000: its first cell is number 4.9e9, its first value number 4.41e10.  A product or a sum
    of the index formed in 32 bits anywhere gives another digest."""
    nx = 70000
    cells = 0.5 * np.arange(nx, dtype=np.float64)[:, None] + np.arange(9, dtype=np.float64)[None, :]
    assert 70000 * nx > 1 << 32
    rows, total = _both(f64, cells, nx, 70000)
    assert rows == [0x7a51a9d7effd116d] and total == rows[0]


def test_known_answers_signed_zeros(f64):
    rows, _ = _both(f64, np.zeros(9), 1, 0)
    assert rows == [0xb0f532d4bdaff080]
    rows, _ = _both(f64, -np.zeros(9), 1, 0)
    assert rows == [0x2f1a53d22b6d97a2]


# ---- against the restatement on states full of edge values ----------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(1, 1), (7, 5), (300, 3)])
@pytest.mark.parametrize("y0", [0, 3, (1 << 40) + 1])
def test_equals_the_restatement_on_edge_values(f64, nx, ny, y0):
    state = ref.edge_state(nx, ny, seed=nx + ny)
    held = set(int(v) for v in ref.bits(state).reshape(-1))
    assert nx * ny < 6 or held >= set(int(v) for v in ref.EDGE_BITS)
    assert np.isnan(state).any() and (nx * ny == 1 or np.isinf(state).any())
    _both(f64, state, nx, y0)


def test_the_state_is_digested_as_it_is(f64):
    """digest_host neither copies a contiguous float64 array nor changes a bit of it (a conversion would quieten signalling NaNs)."""
    state = ref.edge_state(7, 5)
    before = ref.bits(state).copy()
    f64.digest_host(state, 7)
    assert np.array_equal(ref.bits(state), before)
    a, _ = f64.digest_host(state.reshape(-1), 7)
    b, _ = f64.digest_host(state[::1], 7)
    assert np.array_equal(a, b)


# ---- additivity ---------------------------------------------------------------------------------------------------------------------
def test_every_split_of_seven_rows_adds_up(f64):
    nx, ny = 5, 7
    state = ref.edge_state(nx, ny, seed=3)
    whole_rows, whole = f64.digest_host(state, nx)
    for a in range(ny + 1):
        for b in range(a, ny + 1):
            parts = [f64.digest_host(state[lo:hi], nx, lo) for lo, hi in ((0, a), (a, b), (b, ny))]
            assert sum(t for _, t in parts) & MASK == whole, (a, b)
            assert np.array_equal(np.concatenate([r for r, _ in parts]), whole_rows), (a, b)
    rows, total = f64.digest_host(state[:0], nx, 4)          # an empty range
    assert rows.size == 0 and total == 0


# ---- sensitivity --------------------------------------------------------------------------------------------------------------------
def test_one_mantissa_bit_changes_exactly_its_row(f64):
    nx, ny = 6, 5
    state = ref.edge_state(nx, ny, seed=9)
    base, _ = f64.digest_host(state, nx)
    for y, x, k in ((0, 0, 0), (2, 5, 7), (4, 3, 8)):
        other = state.copy()
        ref.bits(other).reshape(ny, nx, 9)[y, x, k] ^= np.uint64(1)
        rows, _ = f64.digest_host(other, nx)
        assert [int(i) for i in np.nonzero(rows != base)[0]] == [y], (y, x, k)


def test_exchanging_two_cells_changes_the_digest(f64):
    """The same multiset of values at other places: in one row (that row's digest alone) and across two rows (both)."""
    nx, ny = 6, 4
    state = np.random.default_rng(1).uniform(0.01, 0.2, (ny, nx, 9))
    base, total = f64.digest_host(state, nx)
    other = state.copy()
    other[1, 2], other[1, 4] = state[1, 4], state[1, 2]
    rows, t = f64.digest_host(other, nx)
    assert [int(i) for i in np.nonzero(rows != base)[0]] == [1] and t != total
    other = state.copy()
    other[0, 3], other[3, 3] = state[3, 3], state[0, 3]
    rows, t = f64.digest_host(other, nx)
    assert [int(i) for i in np.nonzero(rows != base)[0]] == [0, 3] and t != total
    other = state.copy()                                    # two populations of one cell
    other[2, 1, 5], other[2, 1, 6] = state[2, 1, 6], state[2, 1, 5]
    rows, t = f64.digest_host(other, nx)
    assert [int(i) for i in np.nonzero(rows != base)[0]] == [2] and t != total


# ---- the header, the exports --------------------------------------------------------------------------------------------------------
def test_header_is_c99_and_a_c_caller_links(lbm, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''
#include <stdio.h>
#include "lbm_d2q9_f64_digest.h"
int main(void)
{
  double cells[54];
  unsigned long long rows[2] = {0, 0}, digest = 0;
  int i;
  for (i = 0; i < 54; ++i) cells[i] = (1 + i) / 8.0;
  if (lbm_digest64_abi_version() != LBM_DIGEST64_ABI_VERSION || LBM_DIGEST64_ABI_VERSION != 1) return 2;
  if (lbm64_abi_version() != 1 || lbm_rows64_abi_version() != 1 || LBM_ABI_VERSION != 5) return 3;
  if (lbm_digest64_host(cells, 3, 2, 5, rows, &digest)) return 4;
  printf("%016llx %016llx %016llx\\n", rows[0], rows[1], digest);
  if (lbm_digest64_grid(NULL, 0, 1, rows, &digest) != 1) return 5;
  printf("%s\\n", lbm_last_error());
  if (lbm_digest64_rows(NULL, 0, 1, rows, &digest) != 1) return 6;
  printf("%s\\n", lbm_last_error());
  return 0;
}
''')
    exe = tmp_path / "caller"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L",
                        os.path.dirname(lbm.LIB_PATH), "-llbm_d2q9", f"-Wl,-rpath,{os.path.dirname(lbm.LIB_PATH)}", "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert lines[0] == "3d372f979e5dd85a 36adf4c564caeb7d 73e5245d0328c3d7"
    assert lines[1] == "lbm_digest64_grid: null context" and lines[2] == "lbm_digest64_rows: null run"


def test_library_exports_every_declared_digest_symbol(lbm, f64):
    header = open(os.path.join(ROOT, "include", "lbm_d2q9_f64_digest.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lbm_digest64_[a-z_0-9]+)\s*\(", header))
    assert declared == {"lbm_digest64_abi_version", "lbm_digest64_host", "lbm_digest64_grid", "lbm_digest64_rows"}
    nm = subprocess.run(["nm", "-D", "--defined-only", lbm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (lbm_digest64_[a-z_0-9]+)", nm))
    assert declared == exported, declared ^ exported
    assert declared == set(f64.DIGEST_EXPORTS)
    assert f64.load_digest_library().lbm_digest64_abi_version() == 1 == f64.DIGEST_ABI_VERSION
    # the ABIs beside it are as they were: no new name under their prefixes
    assert set(re.findall(r" T (lbm64_[a-z_0-9]+)", nm)) == set(f64.EXPORTS) and len(f64.EXPORTS) == 15
    assert set(re.findall(r" T (lbm_rows64_[a-z_0-9]+)", nm)) == set(f64.ROWS_EXPORTS) and len(f64.ROWS_EXPORTS) == 10
    assert not set(f64.DIGEST_EXPORTS) & (set(f64.EXPORTS) | set(f64.ROWS_EXPORTS) | set(lbm.EXPORTS))
    assert f64.load_library().lbm64_abi_version() == 1 and f64.load_rows_library().lbm_rows64_abi_version() == 1
    assert lbm.load_library().lbm_abi_version() == 5
    assert b"lbm64_row_digest_kernel" in open(lbm.LIB_PATH, "rb").read()      # the device half is in the code object


# ---- the refusals that need no GPU ----------------------------------------------------------------------------------------------------
def _message(lbm):
    return lbm.load_library().lbm_last_error().decode()


def test_host_refusals(lbm, f64):
    lib = f64.load_digest_library()
    cells = np.zeros(2 * 3 * 9)
    rows = np.zeros(2, np.uint64)
    total = C.c_ulonglong(0)
    cp, rp = cells.ctypes.data_as(C.POINTER(C.c_double)), rows.ctypes.data_as(C.POINTER(C.c_ulonglong))
    for args, text in (((cp, 3, 2, 0, None, None), "both output pointers are null"),
                       ((cp, 0, 2, 0, rp, C.byref(total)), "nx must be positive"),
                       ((cp, -3, 2, 0, rp, C.byref(total)), "nx must be positive"),
                       ((cp, 3, -1, 0, rp, C.byref(total)), "negative row count"),
                       ((cp, 3, 2, -1, rp, C.byref(total)), "negative first row"),
                       ((None, 3, 2, 0, rp, C.byref(total)), "null state")):
        assert lib.lbm_digest64_host(*args) != 0, text
        assert _message(lbm).startswith("lbm_digest64_host: ") and text in _message(lbm), (text, _message(lbm))
    # either output alone is enough; no rows is a digest of 0
    assert lib.lbm_digest64_host(cp, 3, 2, 0, rp, None) == 0 and lib.lbm_digest64_host(cp, 3, 2, 0, None, C.byref(total)) == 0
    assert total.value == sum(int(v) for v in rows) & MASK
    total.value = 7
    assert lib.lbm_digest64_host(None, 3, 0, 9, None, C.byref(total)) == 0 and total.value == 0
    with pytest.raises(lbm.LbmError, match="nx must be positive"):
        f64.digest_host(cells, 0)
    with pytest.raises(ValueError, match="whole rows"):
        f64.digest_host(cells[:-1], 3)


def test_cli_refuses_the_switch_without_double_precision(lbm, digests, tmp_path):
    from conftest import deck_paths
    ppath, opath = deck_paths("tiny_8x3", digests)
    base = {k: v for k, v in os.environ.items() if not k.startswith("LBM")}
    for extra in ({}, {"LBM_PRECISION": "float"}):
        r = subprocess.run([lbm.CLI_PATH, ppath, opath], cwd=tmp_path, env={**base, "LBM_DIGEST": "1", **extra}, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "LBM_DIGEST: the state digest is the double-precision mode's, it needs LBM_PRECISION=double" in r.stderr
        assert "state digest:" not in r.stderr and not (tmp_path / "final_state.dat").exists()


def test_device_entry_points_refuse_without_touching_hip(lbm, f64):
    """No context can be made on a machine without a GPU, so what can be checked here is the order: a null context or run is refused
    with its own message whatever the range and the outputs, and on a machine with no GPU nothing about HIP is said.  The refusals of a
    bad range on a live context are in tests/test_f64_digest.py."""
    lib = f64.load_digest_library()
    rows = np.zeros(4, np.uint64)
    total = C.c_ulonglong(0)
    rp = rows.ctypes.data_as(C.POINTER(C.c_ulonglong))
    for entry, text in ((lib.lbm_digest64_grid, "lbm_digest64_grid: null context"), (lib.lbm_digest64_rows, "lbm_digest64_rows: null run")):
        for y_begin, y_end, out, tot in ((0, 4, rp, C.byref(total)), (-1, 4, rp, C.byref(total)), (3, 2, rp, C.byref(total)),
                                         (0, 1 << 30, rp, C.byref(total)), (0, 0, rp, C.byref(total)), (0, 4, None, None)):
            assert entry(None, y_begin, y_end, out, tot) != 0
            assert _message(lbm) == text and "hip" not in _message(lbm).lower()
