"""The chunked read-outs of the double-precision mode with more than one chunk: LBM_TUNE_OBS_CHUNK_CELLS (read when a context is
created) below the size of a whole grid (f64.Grid64) and of a rank's row block (f64.Rows64), so that every copy after the first
starts at a row offset into the device grid and into the caller's array, and the last one is ragged.  The default chunk is 16 M
cells: no other double-precision test gets past its first chunk."""
import numpy as np
import pytest

import f64_ref
from test_f64_rows import BLOCK, U, _bits, _random_state, _synthetic

pytestmark = pytest.mark.gpu

KNOB = "LBM_TUNE_OBS_CHUNK_CELLS"

# (nx, ny, ranks: None for a whole grid, rows per rank, the knob, chunks per rank: (whole ones, rows of the ragged last one))
CASES = [(7, 5, None, [5], 2 * 7 + 3, [(2, 1)]),                    # odd nx, two rows per chunk
         (7, 5, 2, [2, 3], 2 * 7 + 3, [(1, 0), (1, 1)]),
         (258, 33, None, [33], 4 * 258 + 5, [(8, 1)]),              # four rows per chunk
         (258, 33, 4, [9, 8, 8, 8], 4 * 258 + 5, [(2, 1), (2, 0), (2, 0), (2, 0)])]


@pytest.fixture(scope="module")
def f64(lbm):
    from mpilattice_boltzmann_amd import f64 as mod
    mod.load_rows_library()
    return mod


_REFERENCES = {}


def _reference(p, obst):
    """A random positive state and the restatement's three steps from it, once per shape: never written to."""
    key = (p.nx, p.ny)
    if key not in _REFERENCES:
        state = _random_state(p)
        ref3, _, _ = f64_ref.run(p, obst, 3, cells0=state)
        for a in (state, ref3):
            a.setflags(write=False)
        _REFERENCES[key] = (state, ref3)
    return _REFERENCES[key]


def _open(f64, p, obst, nranks):
    return f64.Grid64(p, obst) if nranks is None else f64.Rows64(p, obst, nranks, devices=[0] * nranks)


@pytest.mark.parametrize("nx,ny,nranks,rows,knob,chunks", CASES)
def test_read_outs_in_several_chunks(lbm, f64, monkeypatch, nx, ny, nranks, rows, knob, chunks):
    assert lbm.decompose(ny, nranks or 1)[0] == rows
    per_chunk = knob // nx                              # whole rows per chunk (csrc: chunk_cells)
    assert [(r // per_chunk, r % per_chunk) for r in rows] == chunks and knob % nx != 0
    p, obst = _synthetic(lbm, nx, ny)
    state, ref3 = _reference(p, obst)

    monkeypatch.setenv(KNOB, str(knob))
    with _open(f64, p, obst, nranks) as g:
        g.set_cells(state)
        assert np.array_equal(_bits(g.get_cells()), _bits(state)), "get_cells(set_cells(x)) != x"
        g.run(3)
        cells = g.get_cells()
        obs = g.get_observables()
        tot = g.av_velocity_sum()
    monkeypatch.delenv(KNOB)
    with _open(f64, p, obst, nranks) as g:              # the same calls in one chunk each
        g.set_cells(state)
        g.run(3)
        obs_whole = g.get_observables()

    # a set and a get that shared a wrong offset would pass the round trip; the kernels between them read the grid where it is
    assert np.array_equal(_bits(cells), _bits(ref3)), "set_cells, run(3), get_cells against the restatement"
    assert np.array_equal(_bits(obs), _bits(obs_whole)), "get_observables against a context with the default chunk"
    # tests/test_f64.py test_observables_and_velocity_sum's comparison (test_f64_rows.py's over the ranks): a lane adds
    # ceil(n_r / (b_r * 256)) terms serially, block_sum's nine, then the host adds the ranks' b_r block sums serially
    rank_cells = [r * nx for r in rows]
    blocks = [min(-(-n // BLOCK), 1024) for n in rank_cells]
    bound = (max(-(-n // (b * BLOCK)) for n, b in zip(rank_cells, blocks)) + 9 + sum(blocks)) * U
    exact = f64_ref.velocity_sum_exact(cells, obst)
    print(f"  {nx}x{ny} {'whole' if nranks is None else f'on {nranks} ranks'}, velocity sum: {abs(tot - exact) / exact / U:.2f} x 2^-53 against {bound / U:.0f} x 2^-53")
    assert abs(tot - exact) <= bound * exact
