"""The yardstick of tests/test_terms_sums.py and tests/test_terms_cells.py, checked on the CPU: the oracle's exactly rounded sum
(oracle_exact_sum, oracle_run_sums) against math.fsum, av_exact against it, tests/terms_ref.py's numpy cell entry against the oracle's
per-cell terms, and the census self-check: one free cell's term removed from a step's sum, or counted twice, moves the sum by more than
the bound the device's sums are held to."""
import math

import numpy as np
import pytest

import terms_ref
from conftest import deck_paths

U = 2.0 ** -53


class _Params:
    def __init__(self, nx, ny, max_iters, reynolds_dim, density, accel, omega):
        self.nx, self.ny, self.max_iters, self.reynolds_dim = nx, ny, max_iters, reynolds_dim
        self.density, self.accel, self.omega = density, accel, omega


def _odd_case():
    """12 x 7 with an odd obstacle map: a blocked corner, a blocked run on row ny - 2, single cells elsewhere; from a random state."""
    p = _Params(12, 7, 9, 4, 0.1, 0.02, 1.4)
    obst = np.zeros((7, 12), np.int32)
    obst[0, 0] = obst[6, 11] = obst[5, 3] = obst[5, 4] = obst[5, 5] = obst[2, 7] = obst[3, 0] = obst[4, 11] = obst[1, 6] = 1
    return p, obst, terms_ref.random_state(7, 12, 31)


@pytest.fixture(scope="module")
def cases(oracle, digests):
    """name -> (p, obst, steps, cells0 or None, per-step (ny, nx) terms, sum_exact, av_exact).  rand_64x48 runs from its deck's rest state
    through oracle_run_sums, the 12 x 7 grid from a random state through the same entry and through run_from."""
    out = {}
    ppath, opath = deck_paths("rand_64x48", digests)
    p = oracle.read_params(ppath)
    obst, _ = oracle.read_obstacles(opath, p.nx, p.ny)
    cells0 = np.empty((p.ny, p.nx, 9), np.float32)
    import ctypes as C
    oracle.lib().oracle_init_cells(C.byref(oracle.cparams(p)), oracle._f(cells0), p.ny)
    for name, (p, obst, cells0, from_deck) in {"rand_64x48": (p, obst, cells0, True), "odd_12x7": _odd_case() + (False,)}.items():
        steps = 25
        _, av_from, sums_from, terms = oracle.run_from(p, obst, cells0, steps, sums=True, keep_terms=True)
        cells, av_exact, sum_exact = oracle.run_sums(p, obst, steps, cells0=None if from_deck else cells0)
        # (run_from's av_exact is numpy's sum of the same terms, in numpy's order: not compared)
        assert np.array_equal(sums_from, sum_exact), "the deck route and the run_from route give the same exactly rounded sums"
        out[name] = (p, obst, steps, cells0, terms, sum_exact, av_exact)
    return out


@pytest.mark.parametrize("name", ["rand_64x48", "odd_12x7"])
def test_c_accumulator_equals_fsum(oracle, cases, name):
    p, obst, steps, cells0, terms, sum_exact, av_exact = cases[name]
    free = obst == 0
    for t in range(steps):
        assert sum_exact[t] == math.fsum(terms[t][free].tolist()), (name, t)
        assert np.all(terms[t][~free] == 0)
    # the accumulator alone, on values that cancel and span 130 binades: what a running double sum gets wrong
    rng = np.random.default_rng(9)
    x = rng.standard_normal(50000) * 2.0 ** rng.integers(-70, 60, 50000)
    x = np.concatenate([x, -x[:20000], [1e300, 1.0, -1e300, 2.0 ** -1074]])
    assert oracle.exact_sum(x) == math.fsum(x.tolist())
    assert oracle.exact_sum(np.zeros(0)) == 0.0


@pytest.mark.parametrize("name", ["rand_64x48", "odd_12x7"])
def test_av_exact_within_its_row_sums_of_the_exact_sum(oracle, cases, name):
    """av_exact adds a row's nx terms, then the ny row sums, and multiplies by free_cells_inv: nx + ny - 2 additions of non-negative
    doubles and one product, against one product here: (nx + ny) * 2^-53 relative."""
    p, obst, steps, cells0, terms, sum_exact, av_exact = cases[name]
    inv = np.float64(np.float32(1.0) / np.float32(int(np.sum(obst == 0))))
    ref = sum_exact * inv
    assert np.all(ref > 0)
    rel = np.abs(av_exact - ref) / ref
    print(f"  {name}: av_exact off by at most {rel.max() / U:.2f} x 2^-53 (bound {p.nx + p.ny})")
    assert np.all(rel <= (p.nx + p.ny) * U)


@pytest.mark.parametrize("name", ["rand_64x48", "odd_12x7"])
def test_numpy_cell_entry_equals_the_oracle_terms(oracle, cases, name):
    """terms_ref.cell_terms on the streamed-in populations of the state each step starts from: the oracle's terms, every bit; so are the
    exact-mode msq and rinv of tests/fused_ref.c, which the fused entry shares its moments with."""
    import fused_ref
    p, obst, steps, cells0, terms, sum_exact, av_exact = cases[name]
    cells = cells0
    for t in range(6):
        mine = terms_ref.step_terms(p, obst, cells)
        assert np.array_equal(mine.view(np.uint64), terms[t].view(np.uint64)), (name, t)
        pulled = terms_ref.pulled(terms_ref.accelerated(p, obst, cells))
        msq, rinv = terms_ref.msq_rinv(pulled)
        c_msq, c_rinv = fused_ref.cells_msq_rinv(pulled, "exact")
        assert np.array_equal(msq.view(np.uint32), c_msq.view(np.uint32)) and np.array_equal(rinv.view(np.uint32), c_rinv.view(np.uint32))
        cells, _ = oracle.run_from(p, obst, cells, 1)


def test_fused_step_sums_are_fused_ref_terms_exactly_summed(oracle):
    """terms_ref.StepSums in the fused arithmetic: the same state as fused_ref.run, sums within its row sums of fused_ref.run's."""
    import fused_ref
    p, obst, cells0 = _odd_case()
    ref = terms_ref.StepSums(p, obst, cells0, 7, fused=True)
    cells, sums = fused_ref.run(p, obst, 7, "fused", cells0=cells0)
    assert np.array_equal(cells.view(np.uint32), ref.cells.view(np.uint32))
    assert np.all(np.abs(sums - ref.sums) <= (p.nx + p.ny) * U * ref.sums)
    assert np.array_equal(terms_ref.step_terms(p, obst, cells0, fused=True), ref.terms[0])


def test_census_self_check(oracle):
    """64 x 32, 30 % blocked, from a random state: at every step the smallest free cell's term, taken out of the exact sum or put in
    twice, moves the sum by more than the bound tests/test_terms_sums.py asserts for any family and form but the float one (the largest of
    them: the compensated form's), and at most 0.1 % of the free cells (here: none) carry a term below 8 x that bound."""
    import test_terms_sums as ts
    p = _Params(64, 32, 11, 4, 0.1, 0.005, ts.OMEGA)
    obst = ts.census_obstacles(64, 32, 5, (16, 8), (16, 8))
    ref = terms_ref.StepSums(p, obst, terms_ref.random_state(32, 64, 77), 11)
    rel = max(ts.rel_bound(family, form) for family in ts.TREE_DEPTH for form in ("double", "compensated"))
    assert rel < 2.0 ** -40
    free = obst == 0
    for t in range(11):
        terms = ref.terms[t][free]
        assert np.all(terms > 0)
        bound = rel * ref.sums[t]
        smallest = float(terms.min())
        without = math.fsum(np.delete(terms, np.argmin(terms)).tolist())
        twice = math.fsum(terms.tolist() + [smallest])
        print(f"  step {t}: smallest term {smallest:.3e}, bound {bound:.3e}: {smallest / bound:.1e} x")
        assert ref.sums[t] - without > bound and twice - ref.sums[t] > bound
        assert ref.share_below(t, 8 * bound) == 0.0
