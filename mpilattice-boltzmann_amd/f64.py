"""The double-precision mode: ctypes binding of include/lbm_d2q9_f64.h (same library, liblbm_d2q9.so) and its host mirror.

    from mpilattice_boltzmann_amd import f64
    p = f64.read_params64("input_128x128.params")
    obst, free = lbm.read_obstacles("obstacles_128x128.dat", p.nx, p.ny)
    with f64.Grid64(p, obst) as g:
        av_vels = g.run(p.max_iters)
        print(g.reynolds())
        g.write_values("final_state.dat", "av_vels.dat", av_vels)

The reference's arithmetic with every float object a double (the contract is in the header): whole periodic grids on one GPU, one
step per launch of lbm_step_kernel_f64 or, with `flags=f64.FLAG_TILE_STEPS` on a small grid, several per launch of lbm_tile_kernel_f64,
with `flags=f64.FLAG_MULTI_STEPS` on a large one, several per launch of lbm_multi_kernel_f64 (the same populations, bit for bit);
`flags=f64.FLAG_MULTI_ANY_SIZE` means the same and also takes the large grids that 32 x 16 tiles do not cover exactly.  There is no CPU fallback: a missing library or symbol raises.

`f64.Rows64(p, obst, nranks, devices=None)` is the same grid as `nranks` row blocks over one or several GPUs of this process
(include/lbm_d2q9_f64_rows.h): Grid64's methods, Grid64's populations bit for bit for every rank count.  With
`flags=f64.FLAG_ROWS_MULTI_STEPS`, ranks that 32 x 16 tiles cover advance several steps per launch and exchange
(lbm_rows_multi_kernel_f64): the same populations.  `flags=f64.FLAG_ROWS_MULTI_ANY_SIZE` means the same and also takes the runs
of any even width >= 32 whose every rank owns >= 16 rows, uneven ranks among them, by the kernel's edge-tile form.

`f64.Cols64(p, obst, nranks, devices=None)` is the same grid as `nranks` COLUMN blocks (include/lbm_d2q9_f64_cols.h), for grids much
wider than tall: Rows64's methods, the same populations, K steps per launch and exchange (lbm_cols_multi_kernel_f64).  It takes even
nx, blocks of at least 32 columns and ny >= 16, and refuses everything else.

`g.digest()` of either class gives one 64-bit digest per row of the current state and their sum (include/lbm_d2q9_f64_digest.h), taken
on the device; `f64.digest_host(cells, nx)` the same of an array, `f64.differing_rows(a, b)` the rows in which two objects differ.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import _capi
from ._capi import LbmError, check
from .decks import Params

ABI_VERSION = 1
FLAG_NT_STORES, FLAG_NO_NT_STORES = _capi.FLAG_NT_STORES, _capi.FLAG_NO_NT_STORES
FLAG_TILE_STEPS = 512        # LBM64_FLAG_TILE_STEPS: small grids advance several steps per launch (lbm_tile_kernel_f64); the same populations
FLAG_MULTI_STEPS = 1024      # LBM64_FLAG_MULTI_STEPS: large grids that 32 x 16 tiles cover do (lbm_multi_kernel_f64); the same populations
FLAG_MULTI_ANY_SIZE = 4096   # LBM64_FLAG_MULTI_ANY_SIZE: FLAG_MULTI_STEPS, and large grids of any even width >= 32 and ny >= 16 by the kernel's edge-tile form ("lbm_multi_kernel_f64<K,edge>"); the same populations
FLAG_ROWS_MULTI_STEPS = 2048  # LBM_ROWS64_FLAG_MULTI_STEPS: Rows64 only; ranks that 32 x 16 tiles cover advance K steps per launch and exchange (lbm_rows_multi_kernel_f64); the same populations
FLAG_ROWS_MULTI_ANY_SIZE = 8192  # LBM_ROWS64_FLAG_MULTI_ANY_SIZE: Rows64 only; FLAG_ROWS_MULTI_STEPS, and runs of any even width >= 32 whose every rank owns >= 16 rows by the kernel's edge-tile form ("lbm_rows_multi_kernel_f64<K,edge>"); the same populations


class CParams64(C.Structure):
    """struct lbm64_params."""

    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("max_iters", C.c_int), ("reynolds_dim", C.c_int),
                ("density", C.c_double), ("accel", C.c_double), ("omega", C.c_double)]


_P = C.POINTER
_ctx = C.c_void_p
_SIGNATURES = {
    "lbm64_abi_version": (C.c_int, []),
    "lbm64_read_params": (C.c_int, [C.c_char_p, _P(CParams64)]),
    "lbm64_av_velocity_obs": (C.c_double, [_P(CParams64), _P(C.c_double), _P(C.c_int), C.c_int]),
    "lbm64_reynolds": (C.c_double, [_P(CParams64), C.c_double]),
    "lbm64_write_final_state_obs": (C.c_int, [C.c_char_p, _P(CParams64), _P(C.c_double), _P(C.c_int), C.c_int, C.c_int, C.c_int]),
    "lbm64_write_av_vels": (C.c_int, [C.c_char_p, _P(C.c_double), C.c_int]),
    "lbm64_create": (C.c_int, [_P(_ctx), _P(CParams64), C.c_int, _P(C.c_int), C.c_int, C.c_uint]),
    "lbm64_destroy": (C.c_int, [_ctx]),
    "lbm64_run": (C.c_int, [_ctx, C.c_int, _P(C.c_double)]),
    "lbm64_get_cells": (C.c_int, [_ctx, _P(C.c_double)]),
    "lbm64_set_cells": (C.c_int, [_ctx, _P(C.c_double)]),
    "lbm64_get_observables": (C.c_int, [_ctx, _P(C.c_double)]),
    "lbm64_av_velocity_sum": (C.c_int, [_ctx, _P(C.c_double)]),
    "lbm64_last_run_kernel_ms": (C.c_int, [_ctx, _P(C.c_double), _P(C.c_int)]),
    "lbm64_describe": (C.c_int, [_ctx, C.c_char_p, C.c_size_t, _P(C.c_longlong), _P(C.c_longlong), _P(C.c_longlong)]),
}
EXPORTS = tuple(_SIGNATURES)

_typed = None


def load_library() -> C.CDLL:
    """liblbm_d2q9.so with the lbm64_* prototypes set.  Raises if the library or one of the symbols is absent."""
    global _typed
    if _typed is None:
        lib = _capi.load_library()
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)           # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
        if lib.lbm64_abi_version() != ABI_VERSION:
            raise RuntimeError(f"liblbm_d2q9.so double-precision ABI {lib.lbm64_abi_version()} != binding {ABI_VERSION}: rebuild")
        _typed = lib
    return _typed


def _cparams(p) -> CParams64:
    return CParams64(int(p.nx), int(p.ny), int(p.max_iters), int(p.reynolds_dim), float(p.density), float(p.accel), float(p.omega))


def read_params64(paramfile: str) -> Params:
    """`initialise()`'s parameter-file half (`d2q9-bgk.c:772-803`) with density, accel and omega read as doubles (`%lf`);
    LbmError carries the die() text."""
    lib = load_library()
    cp = CParams64()
    check(lib.lbm64_read_params(os.fsencode(paramfile), C.byref(cp)))
    return Params(cp.nx, cp.ny, cp.max_iters, cp.reynolds_dim, cp.density, cp.accel, cp.omega)


def write_av_vels64(path: str, av_vels: np.ndarray) -> None:
    """av_vels.dat (`d2q9-bgk.c:1127-1139`) from doubles."""
    av = np.ascontiguousarray(av_vels, dtype=np.float64)
    check(load_library().lbm64_write_av_vels(os.fsencode(path), _capi.as_double_ptr(av), av.size))


def write_final_state_obs64(path: str, params, obs: np.ndarray, obstacles: np.ndarray) -> None:
    """final_state.dat (`d2q9-bgk.c:1054-1120`) from `Grid64.get_observables()` output."""
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    obst = np.ascontiguousarray(obstacles, dtype=np.int32)
    cp = _cparams(params)
    check(load_library().lbm64_write_final_state_obs(os.fsencode(path), C.byref(cp), _capi.as_double_ptr(obs), _capi.as_int_ptr(obst), int(params.ny), 0, 0))


class Grid64:
    """Device state of a whole periodic grid in double precision — one `lbm64_ctx`."""

    def __init__(self, params, obstacles: np.ndarray, device: int = 0, flags: int = 0):
        self._lib = load_library()
        self.params = params
        self.obstacles = np.ascontiguousarray(obstacles, dtype=np.int32)
        if self.obstacles.shape != (params.ny, params.nx):
            raise ValueError("obstacles must be (ny, nx)")
        self.free_cells = int(self.obstacles.size - np.count_nonzero(self.obstacles))
        self._cp = _cparams(params)
        self._ctx = _ctx()
        check(self._lib.lbm64_create(C.byref(self._ctx), C.byref(self._cp), self.free_cells, _capi.as_int_ptr(self.obstacles), device, flags))

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._lib.lbm64_destroy(self._ctx)
            self._ctx = None

    def __enter__(self) -> "Grid64":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, n_steps: Optional[int] = None) -> np.ndarray:
        """n_steps iterations (default max_iters); returns av_vels, float64 (n_steps,)."""
        n = self.params.max_iters if n_steps is None else int(n_steps)
        av = np.zeros(max(n, 1), dtype=np.float64)
        check(self._lib.lbm64_run(self._ctx, n, _capi.as_double_ptr(av)))
        return av[:n]

    def get_cells(self) -> np.ndarray:
        """(ny, nx, 9) float64, the reference's AoS layout."""
        cells = np.empty((self.params.ny, self.params.nx, 9), dtype=np.float64)
        check(self._lib.lbm64_get_cells(self._ctx, _capi.as_double_ptr(cells)))
        return cells

    def set_cells(self, cells: np.ndarray) -> None:
        cells = np.ascontiguousarray(cells, dtype=np.float64)
        if cells.size != self.params.ny * self.params.nx * 9:
            raise ValueError("cells must hold ny * nx * 9 doubles")
        check(self._lib.lbm64_set_cells(self._ctx, _capi.as_double_ptr(cells)))

    def get_observables(self) -> np.ndarray:
        """(ny, nx, 4) float64 = {u_x, u_y, u, pressure} per cell, the fluid-cell formula for every cell."""
        obs = np.empty((self.params.ny, self.params.nx, 4), dtype=np.float64)
        check(self._lib.lbm64_get_observables(self._ctx, _capi.as_double_ptr(obs)))
        return obs

    def av_velocity_sum(self) -> float:
        """av_velocity()'s sum over the free cells, summed on the device."""
        tot = C.c_double(0.0)
        check(self._lib.lbm64_av_velocity_sum(self._ctx, C.byref(tot)))
        return tot.value

    def reynolds(self) -> float:
        """calc_reynolds (`d2q9-bgk.c:1005-1007`) of the current state, the sum taken in the reference's cell order on the host."""
        obs = self.get_observables()
        tot = self._lib.lbm64_av_velocity_obs(C.byref(self._cp), _capi.as_double_ptr(obs), _capi.as_int_ptr(self.obstacles), self.params.ny)
        return self._lib.lbm64_reynolds(C.byref(self._cp), tot * (1.0 / self.free_cells))

    def write_values(self, final_state_path: str, av_vels_path: str, av_vels: np.ndarray) -> None:
        """write_values (`d2q9-bgk.c:1054-1139`): both output files."""
        write_final_state_obs64(final_state_path, self.params, self.get_observables(), self.obstacles)
        write_av_vels64(av_vels_path, av_vels)

    def last_run_kernel_ms(self) -> tuple[float, int]:
        """(device ms from the first to the last step kernel of the last run, number of step launches)."""
        ms, n = C.c_double(0.0), C.c_int(0)
        check(self._lib.lbm64_last_run_kernel_ms(self._ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def digest(self, y_begin: Optional[int] = None, y_end: Optional[int] = None) -> tuple[np.ndarray, int]:
        """(row digests uint64 (y_end - y_begin,), their wrap-around sum) of global rows [y_begin, y_end) of the current state (default:
        every row), taken on the device (include/lbm_d2q9_f64_digest.h): 8 bytes per row come back.  The state and the next run's
        results are as without the call."""
        return _device_digest(load_digest_library().lbm_digest64_grid, self._ctx, self.params.ny, y_begin, y_end)

    def describe(self) -> dict:
        name = C.create_string_buffer(256)
        blocks, per_block, nbytes = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        check(self._lib.lbm64_describe(self._ctx, name, 256, C.byref(blocks), C.byref(per_block), C.byref(nbytes)))
        return {"kernel": name.value.decode(), "blocks": blocks.value, "cells_per_block": per_block.value, "state_bytes": nbytes.value}


# ---- row-partitioned runs (include/lbm_d2q9_f64_rows.h): a signature table of their own, beside EXPORTS, which stays as it is ----
ROWS_ABI_VERSION = 1
_ROWS_SIGNATURES = {
    "lbm_rows64_abi_version": (C.c_int, []),
    "lbm_rows64_create": (C.c_int, [_P(_ctx), _P(CParams64), C.c_int, _P(C.c_int), C.c_int, _P(C.c_int), C.c_uint]),
    "lbm_rows64_destroy": (C.c_int, [_ctx]),
    "lbm_rows64_run": (C.c_int, [_ctx, C.c_int, _P(C.c_double)]),
    "lbm_rows64_get_cells": (C.c_int, [_ctx, _P(C.c_double)]),
    "lbm_rows64_set_cells": (C.c_int, [_ctx, _P(C.c_double)]),
    "lbm_rows64_get_observables": (C.c_int, [_ctx, _P(C.c_double)]),
    "lbm_rows64_av_velocity_sum": (C.c_int, [_ctx, _P(C.c_double)]),
    "lbm_rows64_last_run_ms": (C.c_int, [_ctx, _P(C.c_double), _P(C.c_int)]),
    "lbm_rows64_describe": (C.c_int, [_ctx, C.c_char_p, C.c_size_t, _P(C.c_int), _P(C.c_longlong), _P(C.c_longlong), _P(C.c_longlong)]),
}
ROWS_EXPORTS = tuple(_ROWS_SIGNATURES)

_rows_typed = None


def load_rows_library() -> C.CDLL:
    """liblbm_d2q9.so with the lbm64_* and the lbm_rows64_* prototypes set.  Raises if the library or one of the symbols is absent."""
    global _rows_typed
    if _rows_typed is None:
        lib = load_library()
        for name, (res, args) in _ROWS_SIGNATURES.items():
            fn = getattr(lib, name)           # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
        if lib.lbm_rows64_abi_version() != ROWS_ABI_VERSION:
            raise RuntimeError(f"liblbm_d2q9.so row-partition ABI {lib.lbm_rows64_abi_version()} != binding {ROWS_ABI_VERSION}: rebuild")
        _rows_typed = lib
    return _rows_typed


class Rows64:
    """A whole periodic grid in double precision, its rows dealt to `nranks` ranks on one or several GPUs — one `lbm_rows64`.
    `devices`: one HIP ordinal per rank (ranks may share a device), or None: rank r on device r % (device count).  Grid64's methods;
    the populations are Grid64's bits for every rank count.  `flags`: 0, a store form, FLAG_ROWS_MULTI_STEPS (several steps per launch
    and exchange where 32 x 16 tiles cover every rank), FLAG_ROWS_MULTI_ANY_SIZE (the same, and ranks of any size from 16 rows on grids of
    any even width from 32: the kernel's edge-tile form), in any sum."""

    def __init__(self, params, obstacles: np.ndarray, nranks: int, devices=None, flags: int = 0):
        self._lib = load_rows_library()
        self.params = params
        self.nranks = int(nranks)
        self.obstacles = np.ascontiguousarray(obstacles, dtype=np.int32)
        if self.obstacles.shape != (params.ny, params.nx):
            raise ValueError("obstacles must be (ny, nx)")
        self.free_cells = int(self.obstacles.size - np.count_nonzero(self.obstacles))
        self._cp = _cparams(params)
        self._run = _ctx()
        dev = None
        if devices is not None:
            devices = [int(d) for d in devices]
            if len(devices) != self.nranks:
                raise ValueError("devices must name one device per rank")
            dev = (C.c_int * max(len(devices), 1))(*devices)
        check(self._lib.lbm_rows64_create(C.byref(self._run), C.byref(self._cp), self.free_cells, _capi.as_int_ptr(self.obstacles), self.nranks, dev, flags))

    def close(self) -> None:
        if getattr(self, "_run", None):
            self._lib.lbm_rows64_destroy(self._run)
            self._run = None

    def __enter__(self) -> "Rows64":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, n_steps: Optional[int] = None) -> np.ndarray:
        """n_steps iterations (default max_iters) on every rank; returns av_vels, float64 (n_steps,)."""
        n = self.params.max_iters if n_steps is None else int(n_steps)
        av = np.zeros(max(n, 1), dtype=np.float64)
        check(self._lib.lbm_rows64_run(self._run, n, _capi.as_double_ptr(av)))
        return av[:n]

    def get_cells(self) -> np.ndarray:
        """(ny, nx, 9) float64 of the whole grid, the reference's AoS layout."""
        cells = np.empty((self.params.ny, self.params.nx, 9), dtype=np.float64)
        check(self._lib.lbm_rows64_get_cells(self._run, _capi.as_double_ptr(cells)))
        return cells

    def set_cells(self, cells: np.ndarray) -> None:
        cells = np.ascontiguousarray(cells, dtype=np.float64)
        if cells.size != self.params.ny * self.params.nx * 9:
            raise ValueError("cells must hold ny * nx * 9 doubles")
        check(self._lib.lbm_rows64_set_cells(self._run, _capi.as_double_ptr(cells)))

    def get_observables(self) -> np.ndarray:
        """(ny, nx, 4) float64 = {u_x, u_y, u, pressure} per cell, the fluid-cell formula for every cell."""
        obs = np.empty((self.params.ny, self.params.nx, 4), dtype=np.float64)
        check(self._lib.lbm_rows64_get_observables(self._run, _capi.as_double_ptr(obs)))
        return obs

    def av_velocity_sum(self) -> float:
        """av_velocity()'s sum over the free cells, summed on the devices, the blocks' sums added rank after rank."""
        tot = C.c_double(0.0)
        check(self._lib.lbm_rows64_av_velocity_sum(self._run, C.byref(tot)))
        return tot.value

    def reynolds(self) -> float:
        """calc_reynolds (`d2q9-bgk.c:1005-1007`) of the current state, the sum taken in the reference's cell order on the host: the
        bits Grid64.reynolds gives."""
        obs = self.get_observables()
        tot = self._lib.lbm64_av_velocity_obs(C.byref(self._cp), _capi.as_double_ptr(obs), _capi.as_int_ptr(self.obstacles), self.params.ny)
        return self._lib.lbm64_reynolds(C.byref(self._cp), tot * (1.0 / self.free_cells))

    def write_values(self, final_state_path: str, av_vels_path: str, av_vels: np.ndarray) -> None:
        """write_values (`d2q9-bgk.c:1054-1139`): both output files."""
        write_final_state_obs64(final_state_path, self.params, self.get_observables(), self.obstacles)
        write_av_vels64(av_vels_path, av_vels)

    def last_run_ms(self) -> tuple[float, int]:
        """(device ms of the last run: the largest span over the ranks from its first step kernel to its last push, step launches)."""
        ms, n = C.c_double(0.0), C.c_int(0)
        check(self._lib.lbm_rows64_last_run_ms(self._run, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def digest(self, y_begin: Optional[int] = None, y_end: Optional[int] = None) -> tuple[np.ndarray, int]:
        """Grid64.digest's pair for the whole grid's rows [y_begin, y_end), each rank digesting the rows it owns on its device."""
        return _device_digest(load_digest_library().lbm_digest64_rows, self._run, self.params.ny, y_begin, y_end)

    def describe(self) -> dict:
        name = C.create_string_buffer(256)
        nranks, blocks, per_block, nbytes = C.c_int(0), C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        check(self._lib.lbm_rows64_describe(self._run, name, 256, C.byref(nranks), C.byref(blocks), C.byref(per_block), C.byref(nbytes)))
        return {"kernel": name.value.decode(), "nranks": nranks.value, "blocks": blocks.value, "cells_per_block": per_block.value, "state_bytes": nbytes.value}


# ---- state digests (include/lbm_d2q9_f64_digest.h): a signature table of their own, beside EXPORTS and ROWS_EXPORTS, which stay as they are ----
DIGEST_ABI_VERSION = 1
_ull = C.c_ulonglong
_DIGEST_SIGNATURES = {
    "lbm_digest64_abi_version": (C.c_int, []),
    "lbm_digest64_host": (C.c_int, [_P(C.c_double), C.c_int, C.c_int, C.c_longlong, _P(_ull), _P(_ull)]),
    "lbm_digest64_grid": (C.c_int, [_ctx, C.c_int, C.c_int, _P(_ull), _P(_ull)]),
    "lbm_digest64_rows": (C.c_int, [_ctx, C.c_int, C.c_int, _P(_ull), _P(_ull)]),
}
DIGEST_EXPORTS = tuple(_DIGEST_SIGNATURES)

_digest_typed = None


def load_digest_library() -> C.CDLL:
    """liblbm_d2q9.so with the lbm64_*, the lbm_rows64_* and the lbm_digest64_* prototypes set.  Raises if the library or one of the
    symbols is absent."""
    global _digest_typed
    if _digest_typed is None:
        lib = load_rows_library()
        for name, (res, args) in _DIGEST_SIGNATURES.items():
            fn = getattr(lib, name)           # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
        if lib.lbm_digest64_abi_version() != DIGEST_ABI_VERSION:
            raise RuntimeError(f"liblbm_d2q9.so digest ABI {lib.lbm_digest64_abi_version()} != binding {DIGEST_ABI_VERSION}: rebuild")
        _digest_typed = lib
    return _digest_typed


def _as_ull_ptr(a: np.ndarray):
    assert a.dtype == np.uint64 and a.flags.c_contiguous
    return a.ctypes.data_as(_P(_ull))


def digest_host(cells: np.ndarray, nx: int, y0: int = 0) -> tuple[np.ndarray, int]:
    """(row digests uint64 (rows,), their wrap-around sum) of AoS cells in host memory that are global rows [y0, y0 + rows) of a grid
    `nx` cells wide; rows = cells.size / (9 * nx).  No GPU.  The bits of `cells` are digested as they are (NaN payloads, signed zeros)."""
    cells = np.ascontiguousarray(cells, dtype=np.float64)
    nx = int(nx)
    if nx >= 1 and cells.size % (9 * nx) != 0:
        raise ValueError("cells must hold whole rows of nx * 9 doubles")
    rows = cells.size // (9 * nx) if nx >= 1 else 0
    out = np.zeros(max(rows, 1), dtype=np.uint64)
    total = _ull(0)
    check(load_digest_library().lbm_digest64_host(_capi.as_double_ptr(cells), nx, rows, int(y0), _as_ull_ptr(out), C.byref(total)))
    return out[:rows], total.value


def _device_digest(entry, handle, ny: int, y_begin, y_end) -> tuple[np.ndarray, int]:
    y_begin = 0 if y_begin is None else int(y_begin)
    y_end = int(ny) if y_end is None else int(y_end)
    out = np.zeros(max(y_end - y_begin, 1), dtype=np.uint64)
    total = _ull(0)
    check(entry(handle, y_begin, y_end, _as_ull_ptr(out), C.byref(total)))
    return out[:y_end - y_begin], total.value


def differing_rows(a, b) -> list[int]:
    """The global rows whose digests differ between two objects of either class (Grid64, Rows64) on grids of the same shape."""
    if (a.params.nx, a.params.ny) != (b.params.nx, b.params.ny):
        raise ValueError("differing_rows: the two grids differ in shape")
    return [int(y) for y in np.nonzero(a.digest()[0] != b.digest()[0])[0]]


# ---- column-partitioned runs (include/lbm_d2q9_f64_cols.h): a signature table of their own, beside the others, which stay as they are ----
COLS_ABI_VERSION = 1
_COLS_SIGNATURES = {
    "lbm_cols64_abi_version": (C.c_int, []),
    "lbm_cols64_create": (C.c_int, [_P(_ctx), _P(CParams64), C.c_int, _P(C.c_int), C.c_int, _P(C.c_int), C.c_uint]),
    "lbm_cols64_destroy": (C.c_int, [_ctx]),
    "lbm_cols64_run": (C.c_int, [_ctx, C.c_int, _P(C.c_double)]),
    "lbm_cols64_get_cells": (C.c_int, [_ctx, _P(C.c_double)]),
    "lbm_cols64_set_cells": (C.c_int, [_ctx, _P(C.c_double)]),
    "lbm_cols64_get_observables": (C.c_int, [_ctx, _P(C.c_double)]),
    "lbm_cols64_av_velocity_sum": (C.c_int, [_ctx, _P(C.c_double)]),
    "lbm_cols64_last_run_ms": (C.c_int, [_ctx, _P(C.c_double), _P(C.c_int)]),
    "lbm_cols64_describe": (C.c_int, [_ctx, C.c_char_p, C.c_size_t, _P(C.c_int), _P(C.c_longlong), _P(C.c_longlong), _P(C.c_longlong)]),
    "lbm_cols64_digest": (C.c_int, [_ctx, C.c_int, C.c_int, _P(_ull), _P(_ull)]),
}
COLS_EXPORTS = tuple(_COLS_SIGNATURES)

_cols_typed = None


def load_cols_library() -> C.CDLL:
    """liblbm_d2q9.so with the lbm64_* and the lbm_cols64_* prototypes set.  Raises if the library or one of the symbols is absent."""
    global _cols_typed
    if _cols_typed is None:
        lib = load_library()
        for name, (res, args) in _COLS_SIGNATURES.items():
            fn = getattr(lib, name)           # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
        if lib.lbm_cols64_abi_version() != COLS_ABI_VERSION:
            raise RuntimeError(f"liblbm_d2q9.so column-partition ABI {lib.lbm_cols64_abi_version()} != binding {COLS_ABI_VERSION}: rebuild")
        _cols_typed = lib
    return _cols_typed


class Cols64(Rows64):
    """A whole periodic grid in double precision, its columns dealt to `nranks` column blocks on one or several GPUs — one
    `lbm_cols64` (include/lbm_d2q9_f64_cols.h): K steps per launch and exchange (lbm_cols_multi_kernel_f64), for grids much wider than
    tall.  Rows64's arguments and methods; the populations are Grid64's bits for every rank count.  `flags`: 0 or a store form.  Taken:
    even nx, every block at least 32 columns wide, ny >= 16; everything else raises LbmError (Rows64 takes every shape)."""

    def __init__(self, params, obstacles: np.ndarray, nranks: int, devices=None, flags: int = 0):
        self._lib = load_cols_library()
        self.params = params
        self.nranks = int(nranks)
        self.obstacles = np.ascontiguousarray(obstacles, dtype=np.int32)
        if self.obstacles.shape != (params.ny, params.nx):
            raise ValueError("obstacles must be (ny, nx)")
        self.free_cells = int(self.obstacles.size - np.count_nonzero(self.obstacles))
        self._cp = _cparams(params)
        self._run = _ctx()
        dev = None
        if devices is not None:
            devices = [int(d) for d in devices]
            if len(devices) != self.nranks:
                raise ValueError("devices must name one device per rank")
            dev = (C.c_int * max(len(devices), 1))(*devices)
        check(self._lib.lbm_cols64_create(C.byref(self._run), C.byref(self._cp), self.free_cells, _capi.as_int_ptr(self.obstacles), self.nranks, dev, flags))

    def close(self) -> None:
        if getattr(self, "_run", None):
            self._lib.lbm_cols64_destroy(self._run)
            self._run = None

    def __enter__(self) -> "Cols64":
        return self

    def run(self, n_steps: Optional[int] = None) -> np.ndarray:
        """n_steps iterations (default max_iters) on every rank; returns av_vels, float64 (n_steps,)."""
        n = self.params.max_iters if n_steps is None else int(n_steps)
        av = np.zeros(max(n, 1), dtype=np.float64)
        check(self._lib.lbm_cols64_run(self._run, n, _capi.as_double_ptr(av)))
        return av[:n]

    def get_cells(self) -> np.ndarray:
        """(ny, nx, 9) float64 of the whole grid, the reference's AoS layout."""
        cells = np.empty((self.params.ny, self.params.nx, 9), dtype=np.float64)
        check(self._lib.lbm_cols64_get_cells(self._run, _capi.as_double_ptr(cells)))
        return cells

    def set_cells(self, cells: np.ndarray) -> None:
        cells = np.ascontiguousarray(cells, dtype=np.float64)
        if cells.size != self.params.ny * self.params.nx * 9:
            raise ValueError("cells must hold ny * nx * 9 doubles")
        check(self._lib.lbm_cols64_set_cells(self._run, _capi.as_double_ptr(cells)))

    def get_observables(self) -> np.ndarray:
        """(ny, nx, 4) float64 = {u_x, u_y, u, pressure} per cell, the fluid-cell formula for every cell."""
        obs = np.empty((self.params.ny, self.params.nx, 4), dtype=np.float64)
        check(self._lib.lbm_cols64_get_observables(self._run, _capi.as_double_ptr(obs)))
        return obs

    def av_velocity_sum(self) -> float:
        """av_velocity()'s sum over the free cells, summed on the devices, the blocks' sums added rank after rank."""
        tot = C.c_double(0.0)
        check(self._lib.lbm_cols64_av_velocity_sum(self._run, C.byref(tot)))
        return tot.value

    # Inherited from Rows64 as they are, because they touch the run only through methods overridden here or not at all: reynolds and
    # write_values (get_observables and the host half of the library), __exit__ and __del__ (close).  Every method that calls an
    # lbm_rows64_* entry point is overridden: a Cols64 never reaches one.

    def last_run_ms(self) -> tuple[float, int]:
        """(device ms of the last run: the largest span over the ranks from its first launch to its last push, launches:
        ceil(n_steps / K) * nranks)."""
        ms, n = C.c_double(0.0), C.c_int(0)
        check(self._lib.lbm_cols64_last_run_ms(self._run, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def digest(self, y_begin: Optional[int] = None, y_end: Optional[int] = None) -> tuple[np.ndarray, int]:
        """Grid64.digest's pair for the whole grid's rows [y_begin, y_end): each rank digests its columns of them on its device, the
        host adds the ranks' parts."""
        load_cols_library()
        return _device_digest(self._lib.lbm_cols64_digest, self._run, self.params.ny, y_begin, y_end)

    def describe(self) -> dict:
        name = C.create_string_buffer(256)
        nranks, blocks, per_block, nbytes = C.c_int(0), C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        check(self._lib.lbm_cols64_describe(self._run, name, 256, C.byref(nranks), C.byref(blocks), C.byref(per_block), C.byref(nbytes)))
        return {"kernel": name.value.decode(), "nranks": nranks.value, "blocks": blocks.value, "cells_per_block": per_block.value, "state_bytes": nbytes.value}


__all__ = ["ABI_VERSION", "EXPORTS", "ROWS_ABI_VERSION", "ROWS_EXPORTS", "DIGEST_ABI_VERSION", "DIGEST_EXPORTS", "digest_host", "differing_rows", "load_digest_library", "FLAG_NT_STORES", "FLAG_NO_NT_STORES", "FLAG_TILE_STEPS", "FLAG_MULTI_STEPS", "FLAG_MULTI_ANY_SIZE", "FLAG_ROWS_MULTI_STEPS", "FLAG_ROWS_MULTI_ANY_SIZE", "CParams64", "Grid64", "Rows64",
           "LbmError", "load_library", "load_rows_library", "read_params64", "write_av_vels64", "write_final_state_obs64",
           "COLS_ABI_VERSION", "COLS_EXPORTS", "Cols64", "load_cols_library"]
