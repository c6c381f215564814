"""The yardstick of tests/test_readout.py held to things that are not the kernels: known answers of the digest as literals (from a
run of the documented formula, recorded in the issue that asked for these tests), its algebra (additive over rows and column windows)
and its sensitivity (every single bit, swaps, the sign of zero); the velocity sum against the oracle's serial float accumulation,
the observables against the host writer's printed file.  No GPU."""
import itertools

import numpy as np
import pytest

import readout_ref

M64 = 1 << 64


def counting_block():
    """(2, 3, 9): the 54 populations have the bit patterns 0, 1, ..., 53."""
    return np.arange(54, dtype=np.uint32).view(np.float32).reshape(2, 3, 9)


def random_block(rows, ncol, seed):
    """Every bit pattern there is (NaNs, infinities, denormals included): the digest reads bits, not numbers."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, (rows, ncol, 9), dtype=np.uint64).astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("cell0,nxg,want", [(0, 3, 0x4fa0b2b44756c610),
                                            (5 * 7 + 2, 7, 0x98bf01e2cf95ea97),
                                            ((2 ** 20 - 2) * 8192 + 8189, 8192, 0x965eb802a38d84e6)])     # index * 9 past 2^36
def test_digest_known_answers(cell0, nxg, want):
    assert readout_ref.digest(counting_block(), cell0, nxg) == want
    assert readout_ref.digest_rows(counting_block(), cell0, nxg, chunk_rows=1) == want


def test_digest_defaults_are_whole_rows_from_cell_zero():
    b = random_block(5, 7, 1)
    assert readout_ref.digest(b) == readout_ref.digest(b, 0, 7)
    assert readout_ref.digest(b[:0]) == 0 and readout_ref.digest(b[:, :0]) == 0
    with pytest.raises(ValueError):
        readout_ref.digest(b, 0, 6)
    with pytest.raises(ValueError):
        readout_ref.digest(b[..., :8])


def test_digest_is_additive_over_rows_and_column_windows():
    nx, ny = 37, 23
    b = random_block(ny, nx, 2)
    whole = readout_ref.digest(b)
    for cut in (1, 11, ny - 1):
        assert (readout_ref.digest(b[:cut]) + readout_ref.digest(b[cut:], cut * nx, nx)) % M64 == whole
    for xcut in (1, 18, nx - 1):
        assert (readout_ref.digest(b[:, :xcut], 0, nx) + readout_ref.digest(b[:, xcut:], xcut, nx)) % M64 == whole
    # four blocks, as the ranks of a 2 x 2 tile decomposition hold them
    total = 0
    for ys, xs in itertools.product((slice(0, 9), slice(9, ny)), (slice(0, 20), slice(20, nx))):
        total += readout_ref.digest(b[ys, xs], ys.start * nx + xs.start, nx)
    assert total % M64 == whole
    # a block somewhere in a larger grid equals the same rows and columns cut out of that grid
    big = random_block(12, 50, 3)
    inner = readout_ref.digest(big[4:9, 13:30], 4 * 50 + 13, 50)
    rest = big.copy()
    outside = np.ones((12, 50), bool)
    outside[4:9, 13:30] = False
    strips = [(slice(0, 4), slice(0, 50)), (slice(9, 12), slice(0, 50)), (slice(4, 9), slice(0, 13)), (slice(4, 9), slice(30, 50))]
    assert (inner + sum(readout_ref.digest(rest[ys, xs], ys.start * 50 + xs.start, 50) for ys, xs in strips)) % M64 == readout_ref.digest(big)


def test_digest_rows_equals_digest_for_any_chunking():
    b = random_block(24, 19, 4)
    for cell0, nxg in ((0, None), (7 * 31 + 5, 31)):
        want = readout_ref.digest(b, cell0, nxg)
        for chunk in (1, 5, 6, 7, 8, 23, 24, 25, 1000):           # divisors of 24 and not
            assert readout_ref.digest_rows(b, cell0, nxg, chunk_rows=chunk) == want
    with pytest.raises(ValueError):
        readout_ref.digest_rows(b, chunk_rows=0)


def test_digest_sees_every_single_bit_every_swap_and_the_sign_of_zero():
    b = random_block(4, 6, 5)
    base = readout_ref.digest(b, 1234567, 4099)
    seen = {base}
    for (r, x), k, bit in itertools.product(((0, 0), (2, 3), (3, 5)), range(9), range(32)):
        c = b.copy()
        c.view(np.uint32)[r, x, k] ^= np.uint32(1 << bit)
        seen.add(readout_ref.digest(c, 1234567, 4099))
    assert len(seen) == 1 + 3 * 9 * 32                          # 864 flips, 864 further distinct values
    c = b.copy()
    c[1, 2], c[1, 3] = b[1, 3], b[1, 2]                         # two neighbouring cells
    assert readout_ref.digest(c, 1234567, 4099) != base
    c = b.copy()
    c[0, 1], c[3, 1] = b[3, 1], b[0, 1]                         # two cells of one column
    assert readout_ref.digest(c, 1234567, 4099) != base
    c = b.copy()
    c[2, 2, 4], c[2, 2, 7] = b[2, 2, 7], b[2, 2, 4]             # two planes of one cell
    assert readout_ref.digest(c, 1234567, 4099) != base
    assert readout_ref.digest(b, 1234568, 4099) != base         # the same bits one cell further on
    z = np.zeros((1, 1, 9), np.float32)
    m = z.copy()
    m[0, 0, 3] = -0.0
    assert readout_ref.digest(z) != readout_ref.digest(m)


def _serial_float_sum(terms):
    """tot_u += sqrt(...) with a float tot_u (d2q9-bgk.c:748): each step is (float)((double)tot_u + term)."""
    acc = np.float32(0.0)
    for v in terms:
        acc = np.float32(np.float64(acc) + v)
    return float(acc)


def test_velocity_terms_and_sum_against_the_oracle(lbm, oracle):
    """A deck state after some steps: the terms, added in cell order into a float as the reference does, give the oracle's float bit
    for bit (so each term is the oracle's); their exactly rounded sum differs from that float by what n serial float additions of
    non-negative terms allow, (n - 1) * 2^-24 relative (each rounds the running sum, which is at most the total)."""
    p = lbm.Params(64, 48, 40, 4, 0.1, 0.005, 1.7)
    obst = lbm.synthetic_obstacles(64, 48, 0.1, 11, True)
    cells, _, _ = oracle.run(p, obst, 40)
    terms = readout_ref.velocity_terms(cells)
    assert terms.dtype == np.float64 and terms.shape == (48, 64)
    free = obst == 0
    want = oracle.av_velocity_sum(p, cells, obst)
    assert want > 0
    assert _serial_float_sum(terms[free]) == want
    exact = readout_ref.velocity_sum(cells, obst)
    n = int(free.sum())
    assert abs(exact - want) <= (n - 1) * 2.0 ** -24 * exact
    assert abs(exact - float(np.sum(terms[free]))) <= 64 * 2.0 ** -53 * exact          # (numpy's pairwise sum: a sanity check of fsum's use)
    # blocked cells are left out, whatever they hold
    poisoned = cells.copy()
    poisoned[~free] = np.nan
    assert readout_ref.velocity_sum(poisoned, obst) == exact
    # the density is summed left to right: a state where any other order gives another float
    odd = np.zeros((1, 1, 9), np.float32)
    e = 2.0 ** -24
    odd[0, 0] = [1.0, 0.5, e, 0, e, 0, 0, 0, 0]                      # (1.5 + e) + e = 1.5 in float (ties to even); 1.5 + (e + e) = 1.5 + 2^-23
    ux = np.float32(0.5) / np.float32(1.5)                           # u_y = (e - e) / rho = 0
    ux_other = np.float32(0.5) / np.float32(1.5 + 2.0 ** -23)
    assert ux != ux_other
    assert readout_ref.velocity_terms(odd)[0, 0] == float(np.sqrt(np.float64(ux * ux)))


def test_velocity_sum_bound_is_the_documented_one():
    assert readout_ref.velocity_sum_bound(1536 * 1024) == (6 + 8 + 1024) * 2.0 ** -53         # 1.15e-13
    assert readout_ref.velocity_sum_bound(64 * 48) == (1 + 8 + 12) * 2.0 ** -53
    assert readout_ref.velocity_sum_bound(262144) == (1 + 8 + 1024) * 2.0 ** -53
    assert readout_ref.velocity_sum_bound(262145) == (2 + 8 + 1024) * 2.0 ** -53


def _parse_final_state(path, ny, nx):
    """final_state.dat (d2q9-bgk.c:1115: "%d %d %.12E %.12E %.12E %.12E %d") -> (ny, nx, 4) float32, the sign of each printed NaN, and the
    obstacle column.  13 significant digits name a float32 uniquely."""
    vals = np.empty((ny, nx, 4), np.float32)
    nan_sign = np.zeros((ny, nx, 4), bool)
    blocked = np.empty((ny, nx), np.int32)
    with open(path) as fh:
        for line in fh:
            t = line.split()
            x, y = int(t[0]), int(t[1])
            for j, tok in enumerate(t[2:6]):
                vals[y, x, j] = np.float32(float(tok))
                nan_sign[y, x, j] = tok.upper() == "-NAN"
            blocked[y, x] = int(t[6])
    return vals, nan_sign, blocked


def test_observables_are_what_the_host_writer_prints(lbm, tmp_path):
    rng = np.random.default_rng(3)
    nx, ny = 48, 20
    p = lbm.Params(nx, ny, 8, 4, 0.1, 0.02, 1.6)
    obst = lbm.synthetic_obstacles(nx, ny, 0.08, 9, False)
    obst[0, :6] = 0
    cells = (rng.random((ny, nx, 9), dtype=np.float32) * 0.02 + 0.004).astype(np.float32)
    cells[0, 0] = 0.0                                            # rho = 0: 0 / 0 (the reference prints -NAN), pressure 0
    cells[0, 1] = [1e-45, 0, 0, 0, 0, 0, 0, 0, 0]                # a denormal density
    cells[0, 2] = [-1.0, 0.5, 0, 0, 0, 0, 0, 0, 0]               # a negative density
    cells[0, 3] = [0, 0.25, 0, -0.25, 0, 0, 0, 0, 0]             # rho = 0 with a numerator: +inf, and u_y = 0 / 0
    cells[0, 4] = [np.inf, 0, 0, 0, 0, 0, 0, 0, -np.inf]         # inf - inf: a NaN generated from non-NaN populations
    cells[0, 5] = [-0.0] * 9                                     # 0.0f + -0.0f = +0.0f
    obs = readout_ref.observables(cells)
    assert obs.dtype == np.float32 and obs.shape == (ny, nx, 4)
    path = str(tmp_path / "final_state.dat")
    lbm.write_final_state(path, p, cells, obst)
    printed, nan_sign, blocked = _parse_final_state(path, ny, nx)
    assert np.array_equal(blocked, obst)
    free = obst == 0
    nan = np.isnan(obs)
    assert nan[0, 0, :3].all() and not nan[0, 0, 3] and nan[0, 3, 1] and nan[0, 4].all()
    assert np.array_equal(np.isnan(printed)[free], nan[free])
    assert np.array_equal(obs.view(np.uint32)[free & ~nan.any(axis=-1)], printed.view(np.uint32)[free & ~nan.any(axis=-1)])
    ok = free[..., None] & ~nan
    assert np.array_equal(obs.view(np.uint32)[ok], printed.view(np.uint32)[ok])
    # every NaN here comes from non-NaN populations: the bits the kernel documents, printed with the sign x86 gives them
    assert np.all(obs.view(np.uint32)[nan] == 0xFFC00000) and nan_sign[free[..., None] & nan].all()
    # the writer's override for blocked cells (:1076-1080) is the writer's, not part of the observables
    assert np.all(printed[~free][:, :3] == 0) and np.all(printed[~free][:, 3] == np.float32(0.1) * (np.float32(1.0) / np.float32(3.0)))
    # ... and the same floats feed the host epilogue: u_x, u_y in, av_velocity()'s float out
    assert lbm.av_velocity_obs(p, obs[1:], obst[1:]) == lbm.av_velocity_host(p, cells[1:], obst[1:])
    assert lbm.av_velocity_obs(p, obs[1:], obst[1:]) == _serial_float_sum(readout_ref.velocity_terms(cells[1:])[free[1:]])
