"""finish_cell_f64 (csrc/kernels/step64.h), the per-cell function of every double-precision kernel, held to the CPU restatement's
f64_ref_cells (tests/f64_ref.c) outside the regime a lattice run stays in: populations that are denormal, zero, negative, huge, infinite
or NaN, densities that cancel, and roots and quotients in every binade.  scripts/experiments/cell64_probe.hip includes the shipped header
and runs the function with one cell per lane; the classes below, 2^20 cells each with fixed seeds, go through it in one child process.

The comparison rule: the sets of NaNs are equal, and wherever the reference holds a number (infinities and both zeros are numbers) the 64
bits are equal.  The sign and payload of a NaN that arithmetic made are not compared (x86 and gfx950 make different default NaNs); at
blocked cells, where no arithmetic happens, every bit is compared.  Terms are compared as populations are.  No tolerance anywhere.

What each class reaches is counted from the reference alone (test_classes_reach_what_they_are_for: no GPU) so that a generator that
drifted into the benign regime fails there, not silently."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import f64_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 20
OMEGA = 1.85
E_MIN, E_MAX = -1074, 1023            # the exponent of the smallest denormal and of the largest finite double


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _make(e, sig, negative=None):
    """The double 2^e * (1 + sig / 2^52) for e >= -1022; below that the denormal with its leading bit at 2^e and as many of sig's high bits
    as fit.  Built as bit patterns: no rounding, no arithmetic."""
    e = np.asarray(e, np.int64)
    sig = np.asarray(sig, np.uint64) & np.uint64((1 << 52) - 1)
    assert e.min() >= E_MIN and e.max() <= E_MAX
    normal = (np.maximum(e, -1022) + 1023).astype(np.uint64) << np.uint64(52) | sig
    shift = np.clip(-1022 - e, 0, 63).astype(np.uint64)
    denormal = (np.uint64(1 << 52) | sig) >> shift
    b = np.where(e >= -1022, normal, denormal)
    if negative is not None:
        b = b | (np.asarray(negative, np.uint64) << np.uint64(63))
    return b.view(np.float64)


def _sig(rng, shape):
    return rng.integers(0, 1 << 52, shape, dtype=np.uint64)


def _exponent(x):
    """floor(log2 |x|) for finite non-zero x, denormals included."""
    m, e = np.frexp(np.abs(x))
    return e.astype(np.int64) - 1


def _rest(density):
    return np.array([density * 4.0 / 9.0] + [density / 9.0] * 4 + [density / 36.0] * 4)


def _class_a(rng, density=0.1):
    return _rest(density)[None, :] * rng.uniform(0.8, 1.2, (N, 9))


def _class_b(rng):
    """One exponent per cell, uniform over [-1070, 1020]; each population within 3 binades of it with a random significand; the first half
    of the class positive, the second half with random signs.  Uniform exponents alone put 0.35 % of the cells where an output is a
    denormal (below 2^-1024 the density's reciprocal is infinite and the cell NaN), so every sixteenth cell takes its exponent from
    [-1028, -1016] instead, the edge of the normal numbers."""
    cell = rng.integers(-1070, 1021, (N, 1))
    edge = rng.integers(-1028, -1015, (N, 1))
    e = np.where((np.arange(N) % 16 == 0)[:, None], edge, cell) + rng.integers(-3, 4, (N, 9))
    neg = rng.integers(0, 2, (N, 9))
    neg[:N // 2] = 0
    return _make(np.clip(e, E_MIN, E_MAX), _sig(rng, (N, 9)), neg)


def _class_c(rng):
    """in[8] = -(in[0] + ... + in[7]), the sum as collide() adds it, moved by 0, +-1 or +-2 units in its last place: the density is exactly
    zero or a few ulps of a summand, of either sign.  On 40 % of the cells the populations are near 2^-1000 and that ulp is a denormal."""
    e = np.where(rng.random((N, 1)) < 0.4, rng.integers(-1020, -974, (N, 1)), rng.integers(-20, 21, (N, 1)))
    pops = np.empty((N, 9))
    pops[:, :8] = np.ldexp(rng.uniform(0.5, 1.5, (N, 8)), e)
    s = np.zeros(N)
    for k in range(8):
        s = s + pops[:, k]
    moved = (_bits(s).astype(np.int64) + rng.integers(-2, 3, N)).astype(np.uint64)
    pops[:, 8] = (moved | np.uint64(1 << 63)).view(np.float64)
    return pops


SPECIALS = np.array([0x0000000000000000, 0x8000000000000000,      # +-0
                     0x0000000000000001, 0x8000000000000001,      # +-5e-324
                     0x000FFFFFFFFFFFFF, 0x800FFFFFFFFFFFFF,      # +- the largest denormal
                     0x0010000000000000, 0x8010000000000000,      # +- the smallest normal
                     0x3FF0000000000000, 0xBFF0000000000000,      # +-1
                     0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF,      # +- the largest finite
                     0x7FF0000000000000, 0xFFF0000000000000,      # +-inf
                     0x7FF8000000000000,                          # a quiet NaN
                     0xFFF4000000ABCDEF], np.uint64)              # a signalling NaN with a payload


def _class_d(rng):
    pops = SPECIALS[rng.integers(0, SPECIALS.size, (N, 9))]
    # Cell 0: nine times -0.0.  The kernel's density starts from t[0] + t[1] and is -0.0, the restatement's starts from +0.0 and is +0.0;
    # 1 / rho is -inf on one side and +inf on the other, but every free-cell output is inf * 0 = NaN on both, and so is the term.
    pops[0] = np.uint64(1 << 63)
    return pops.view(np.float64)


def _class_e(rng):
    """Only in[0], in[1], in[2] are non-zero: mx = in[1], my = in[2], so msq = in[1]^2 + in[2]^2 lands in a binade chosen per cell, each
    from 2^-1074 to 2^1023 equally often; in[0] = 2^j with j 60 above the larger of the two exponents, so that rho == in[0], rinv == 2^-j
    exactly and the term's significand is the root's."""
    E = E_MIN + np.arange(N) % (E_MAX - E_MIN + 1)                     # the binade msq is aimed at
    half = E // 2
    r = np.sqrt(rng.uniform(1.0, 2.0, N) * np.where(E % 2 != 0, 2.0, 1.0))     # sqrt(u * 2^E) = r * 2^half
    theta = rng.uniform(0.0, 2.0 * np.pi, N)
    pops = np.zeros((N, 9))
    pops[:, 1] = np.ldexp(r * np.cos(theta), half)
    pops[:, 2] = np.ldexp(r * np.sin(theta), half)
    pops[:, 0] = np.ldexp(1.0, half + 61)
    return pops


def _class_f(rng):
    """in[0] = r: each binade from 2^-1074 to 2^1023 equally often, the significand 1, 1 + ulp, all ones (2 - ulp) or random, either sign.
    in[1] = 2^k with k = e_r - 60 clipped to [-537, 511]: msq = 2^2k and its root are exact, so term = 2^k * (1 / rho) is a normal number
    with the quotient's significand.  Where r is above 2^-477 the density is r itself; below that 2^k dominates it.
    The last eighth of the class brings tiny r to the division by another route: in[1] = 2^k and in[3] = -2^k cancel in the density
    before in[4] = r is added, with r from 2^-1030 up to 2^-900 (below 2^-1022 denormal; below 2^-1024 the quotient is infinite)."""
    e = E_MIN + np.arange(N) % (E_MAX - E_MIN + 1)
    kind = rng.integers(0, 4, N)
    sig = np.select([kind == 0, kind == 1, kind == 2], [np.uint64(0), np.uint64(1), np.uint64((1 << 52) - 1)], _sig(rng, N))
    pops = np.zeros((N, 9))
    pops[:, 0] = _make(e, sig, rng.integers(0, 2, N))
    pops[:, 1] = np.ldexp(1.0, np.clip(e - 60, -537, 511))
    tail = np.arange(N) >= N - N // 8
    m = int(tail.sum())
    e_t = -1030 + np.arange(m) % 131
    pops[tail] = 0.0
    pops[tail, 1] = 2.0 ** -500
    pops[tail, 3] = -(2.0 ** -500)
    pops[tail, 4] = _make(e_t, sig[tail], rng.integers(0, 2, m))
    return pops


W_BENIGN = (0.1, 0.005)              # density and accel behind w1, w2
W_DENORMAL = (1e-305, 0.005)         # w1 = 5.6e-309, w2 = 1.4e-309: `out[3] - w1 > 0.0` decides on a denormal difference

# name: (generator, seed, (density, accel) of the weights, share of blocked cells)
CLASSES = {
    "A": (_class_a, 101, W_BENIGN, 0.0),
    "B": (_class_b, 102, W_BENIGN, 0.0),
    "C": (_class_c, 103, W_BENIGN, 0.0),
    "D": (_class_d, 104, W_BENIGN, 0.25),
    "E": (_class_e, 105, W_BENIGN, 0.0),
    "F": (_class_f, 106, W_BENIGN, 0.0),
    # the control state at a density of 5e-308, where out[3] is about w1
    "A_denormal_w": (lambda rng: _class_a(rng, density=5e-308), 107, W_DENORMAL, 0.0),
    "B_denormal_w": (_class_b, 108, W_DENORMAL, 0.0),
}

_cache = {}


def _class(name):
    """pops (N, 9), blocked (N,), accel (N,), (w1, w2), and the reference: out (N, 9), term (N,), mom (N, 2).  Once per process, read-only."""
    if name not in _cache:
        gen, seed, dens_accel, p_blocked = CLASSES[name]
        rng = np.random.default_rng(seed)
        pops = np.ascontiguousarray(gen(rng), np.float64)
        blocked = (rng.random(N) < p_blocked).astype(np.int32)
        blocked[0] = 0
        accel = rng.integers(0, 2, N).astype(np.int32)
        w = f64_ref.accel_weights(*dens_accel)
        with np.errstate(all="ignore"):
            ref = f64_ref.cells_each(pops, blocked, accel, OMEGA, w[0], w[1], moments=True)
        for a in (pops, blocked, accel) + ref:
            a.setflags(write=False)
        _cache[name] = (pops, blocked, accel, w) + ref
    return _cache[name]


def _denormal(x):
    return (x != 0.0) & (np.abs(x) < 2.0 ** -1022)


def test_classes_reach_what_they_are_for():
    """From the reference alone: the share of each class that lands where the class is meant to land.  Printed, then asserted."""
    share = {}
    pops, blocked, accel, w, out, term, mom = _class("A")
    share["A: cells holding a NaN"] = (float(np.mean(np.isnan(out).any(axis=1) | np.isnan(term))), "==", 0.0)

    pops, blocked, accel, w, out, term, mom = _class("B")
    share["B: cells with a NaN output"] = (float(np.mean(np.isnan(out).any(axis=1))), "<=", 0.35)
    share["B: cells with 0 < msq < 2^-767"] = (float(np.mean((mom[:, 1] > 0.0) & (mom[:, 1] < 2.0 ** -767))), ">=", 0.05)
    share["B: cells with a denormal output"] = (float(np.mean(_denormal(out).any(axis=1))), ">=", 0.005)

    pops, blocked, accel, w, out, term, mom = _class("C")
    rho = mom[:, 0]
    share["C: cells with rho == 0"] = (float(np.mean(rho == 0.0)), ">=", 0.10)
    share["C: cells with rho denormal"] = (float(np.mean(_denormal(rho))), ">=", 0.10)
    share["C: cells with rho < 0"] = (float(np.mean(rho < 0.0)), ">=", 0.10)

    pops, blocked, accel, w, out, term, mom = _class("D")
    share["D: blocked cells"] = (float(np.mean(blocked != 0)), ">=", 0.24)
    assert np.all(_bits(pops[0]) == np.uint64(1 << 63)) and blocked[0] == 0 and mom[0, 0] == 0.0 and not np.signbit(mom[0, 0])
    assert np.isnan(out[0]).all() and np.isnan(term[0])
    for s in SPECIALS:
        assert np.count_nonzero(_bits(pops) == s) > N // 4

    for name in ("E", "F"):
        pops, blocked, accel, w, out, term, mom = _class(name)
        ok = np.isfinite(term) & (term != 0.0) & ~_denormal(term)
        share[f"{name}: cells with a finite, normal, non-zero term"] = (float(np.mean(ok)), ">=", 0.90)
        x = mom[:, 1] if name == "E" else pops[:, 0]          # E: the squared momentum the root is taken of; F: r
        x = x[np.isfinite(x) & (x != 0.0)]
        hits = np.bincount(_exponent(x) - E_MIN, minlength=E_MAX - E_MIN + 1)
        assert hits.size == E_MAX - E_MIN + 1
        share[f"{name}: fewest hits of a binade from 2^-1074 to 2^1023"] = (float(hits.min()), ">=", 100.0)
    pops, blocked, accel, w, out, term, mom = _class("E")
    below = (mom[:, 1] > 0.0) & (mom[:, 1] < 2.0 ** -767)
    for parity in (0, 1):
        near = below & (_exponent(np.where(below, mom[:, 1], 1.0)) >= -775) & (_exponent(np.where(below, mom[:, 1], 1.0)) % 2 == parity)
        share[f"E: cells with msq in [2^-775, 2^-767), exponent parity {parity}"] = (float(near.sum()), ">=", 100.0)
    assert np.all(pops[:, 0] == mom[:, 0])                        # rho == in[0], a power of two
    pops, blocked, accel, w, out, term, mom = _class("F")
    rho = mom[:, 0]
    share["F: cells with a denormal rho whose reciprocal is finite"] = (float(np.sum(_denormal(rho) & np.isfinite(term))), ">=", 1000.0)
    share["F: cells with |rho| >= 2^1022 (a denormal reciprocal)"] = (float(np.sum(np.abs(rho) >= 2.0 ** 1022)), ">=", 400.0)

    for name in ("A_denormal_w", "B_denormal_w"):
        pops, blocked, accel, w, out, term, mom = _class(name)
        assert 0.0 < w[1] < w[0] < 2.0 ** -1022
        # out[3] before the accelerate: the same cells without it
        with np.errstate(all="ignore"):
            plain, _ = f64_ref.cells_each(pops, blocked, np.zeros(N, np.int32), OMEGA, w[0], w[1])
            diff = plain[:, 3] - w[0]
        share[f"{name}: cells where out[3] - w1 is a non-zero denormal"] = (float(np.mean(_denormal(diff))), ">=", 0.01)

    for what, (value, op, limit) in share.items():
        print(f"  {what}: {value:.6g} (asserted {op} {limit:g})")
    for what, (value, op, limit) in share.items():
        assert {"==": value == limit, "<=": value <= limit, ">=": value >= limit}[op], (what, value, op, limit)


PROBE_SRC = os.path.join(ROOT, "scripts", "experiments", "cell64_probe.hip")


def probe_flags():
    """The flags the library compiles lbm_f64.hip with, from the build itself (build.py: --offload-arch=gfx950 and COMMON).
    The package's `build` attribute is build.py's function, not the module, and importing the submodule by name would rebind it to the
    module for every later caller of pkg.build(): the module is taken from sys.modules, where the package's own import left it."""
    import sys
    import mpilattice_boltzmann_amd as pkg
    flags = ["--offload-arch=gfx950", *sys.modules[pkg.build.__module__].COMMON]
    assert "-ffp-contract=off" in flags and "-O3" in flags
    return flags


def test_probe_compiles_for_gfx950(tmp_path):
    """No GPU: only that the probe cross-compiles with the library's flags, so that a typo cannot turn the GPU test red."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    subprocess.run([hipcc, *probe_flags(), PROBE_SRC, "-o", str(tmp_path / "cell64_probe")], check=True, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def probed(tmp_path_factory):
    """Compile the probe, write every class, run them all in ONE fresh child process under a timeout; returns name -> (out, term)."""
    tmp = tmp_path_factory.mktemp("cell64")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp / "cell64_probe")
    subprocess.run([hipcc, *probe_flags(), PROBE_SRC, "-o", exe], check=True, capture_output=True, timeout=300)
    args = []
    for name in CLASSES:
        pops, blocked, accel, w = _class(name)[:4]
        with open(tmp / f"{name}.in", "wb") as fh:
            fh.write(np.uint64(N).tobytes() + np.array([OMEGA, w[0], w[1]], np.float64).tobytes())
            fh.write(pops.tobytes() + blocked.astype(np.uint8).tobytes() + accel.astype(np.uint8).tobytes())
        args += [str(tmp / f"{name}.in"), str(tmp / f"{name}.out")]
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for name in CLASSES:
        raw = np.fromfile(tmp / f"{name}.out", np.float64)
        assert raw.size == N * 10
        got[name] = (raw[:N * 9].reshape(N, 9), raw[N * 9:])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CLASSES))
def test_device_cell_function_equals_the_restatement(probed, name):
    pops, blocked, accel, w, ref_out, ref_term, mom = _class(name)
    got_out, got_term = probed[name]
    for what, ref, got in (("populations", ref_out, got_out), ("terms", ref_term, got_term)):
        nan_ref, nan_got = np.isnan(ref), np.isnan(got)
        wrong_nan = np.argwhere(nan_ref != nan_got)
        differ = np.argwhere(~nan_ref & ~nan_got & (_bits(ref) != _bits(got)))
        print(f"  {name} {what}: {int(nan_ref.sum())} of {ref.size} NaN in the reference; {len(wrong_nan)} NaNs misplaced, {len(differ)} numbers differ")
        for idx in list(wrong_nan[:3]) + list(differ[:3]):
            c = int(idx[0])
            print(f"    cell {c}: in {[hex(int(v)) for v in _bits(pops[c])]} blocked {blocked[c]} accel {accel[c]}: "
                  f"reference {hex(int(_bits(ref)[tuple(idx)]))}, device {hex(int(_bits(got)[tuple(idx)]))} at {tuple(idx)}")
        assert len(wrong_nan) == 0 and len(differ) == 0, f"class {name}, {what}"
    held = blocked != 0                                # no arithmetic: every bit, NaN payloads and signs included
    assert np.array_equal(_bits(got_out[held]), _bits(ref_out[held])) and np.all(_bits(got_term[held]) == 0)
    if name == "A":
        assert not np.isnan(got_out).any() and not np.isnan(got_term).any()
