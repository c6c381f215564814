"""finish_pair_lo<TERMS> (csrc/kernels/common.h), the sum|u| term code of lbm_tile_kernel and lbm_multi_kernel, held per x-pair to
tests/terms_ref.py in every form the library builds: kTermsDouble, kTermsFloat, kTermsCompensated, and the two of the fused arithmetic.
scripts/experiments/terms_probe.hip includes the shipped header and runs the function with one pair per lane; the classes below, 2^18
pairs each with fixed seeds, go through it in one child process.  No reference value comes from the device.

Notation: u = 2^-24 (half an ulp of a float, relative), m = msq, sigma = sqrt(m) (the real number), ref = the double-form term
fl64(fl64(sqrt(m)) * rinv), which is sigma * rinv within 2^-52 relative.  The AMD instruction set reference gives V_SQRT_F32 and V_RSQ_F32
"1ULP accuracy, denormals are flushed": a result is within one unit in its last place of the true one, i.e. within 2^-23 relative.

DOUBLE FORM (also with the fused msq).  The pair's term is (skip & 1 ? 0 : t0) + (skip & 2 ? 0 : t1) with t_j = ref of cell j: every bit,
NaNs compared by place.

FLOAT FORM.  tf = fl32(v_sqrt_f32(m) * rinv): the root within 2^-23, the product within u, the reference within 2^-52, so
  |tf - ref| <= B_FLOAT * ref,   B_FLOAT = (2^-23 + 2^-24) (1 + 2^-20)
for m >= 2^-126 with rinv and tf normal numbers; a pair whose two cells count adds them in float, one more u of the pair's sum.
Below 2^-126 the instruction flushes its argument ("denormals are flushed"): the root, and with it the term, is exactly 0 — what the
device does is recorded in profiles/r13/terms_probe.txt and pinned here (FLOAT_ROOT_OF_A_DENORMAL_IS_ZERO).

COMPENSATED FORM, m >= 2^-126, rinv normal, 2^-125 <= |ref| <= 2^126 (so that p is a normal number).  The seven operations:
  y  = v_rsq_f32(m)            = (1 + d) / sigma,             |d| <= 2^-23
  s  = fl(m * y)               = sigma (1 + a'),              |a'| <= a = 1.5 * 2^-23 + 2^-47
  r  = fma(-s, s, m)           = -sigma^2 (2 a' + a'^2) (1 + e2) + eta,   |e2| <= u; eta: see below
  c  = fl(fl(r * y) * 0.5)     = r y (1 + e3) / 2,            |e3| <= u (the halving is exact)
  p  = fl(s * rinv)
  e  = fma(s, rinv, -p)        = s rinv - p exactly (the error of a float product is a float) + eta'
  lo = fma(c, rinv, e)         = (c rinv + e)(1 + e4),        |e4| <= u
so s + c - sigma = -sigma [a'^2 / 2 + (a' + a'^2 / 2) th], 1 + th = (1 + e2)(1 + d)(1 + e3), |th| <= 2^-22 (1 + 2^-21):
  |s + c - sigma| <= sigma (1.125 + 3) 2^-46 (1 + 2^-20)
and p + lo = (s + c) rinv + e4 (c rinv + e) with |c rinv + e| <= (a + u)(1 + 2^-20) sigma |rinv| = 2^-22 (1 + 2^-19) sigma |rinv|: one more
2^-46.  Against ref (2^-52 from sigma rinv):
  |hi + lo - ref| <= B_COMP |ref| + A,   B_COMP = 5.125 * 2^-46 (1 + 2^-18) + 2^-51 = 2^-43.63.
A is what underflow adds, with float denormals KEPT (the build as it is: the probe reports it and the test asserts it): a result below
2^-126 is rounded to a multiple of 2^-149, an absolute error of at most 2^-150 instead of a relative u.  That can happen to r (eta; |r| is
about 2^-22 m, and the exact residual has bits down to 2^-47 m), to e (eta') and to lo:
  A = 2^-150 (y / 2) |rinv| (1 + 2^-22) + 2^-150 + 2^-150  <=  2^-151 (1 + 2^-21) |rinv| / sigma + 2^-149.
Relative to ref the first part is 2^-151 / m: 2^-47 at m = 2^-104, where the form stops being accurate to 2^-44, and 2^-25 at m = 2^-126:
the same inequality is the "within float accuracy" bound of the range 2^-126 <= m < 2^-104 (the residual there is a few denormal quanta).
The CPU emulation with an ideal reciprocal root saw 2^-45.9 above 2^-104 and 2^-25 at 2^-126; the measured maxima per binade stand in
profiles/r13/terms_probe.txt.  B_COMP is not taken from them.

COMPENSATED FORM, 0 < m < 2^-126: the guard fmaxf(m, 2^-126) makes y = 2^63, s = sigma q (q = sigma 2^63 < 1) and the sum
ref q (3 - q^2) / 2: an under-estimate, never negative.  Required: 0 <= hi + lo <= ref (1 + 2^-23).
m = 0 with a finite rinv: exactly 0.  m = inf: NaN (the reference has inf).

A pair whose two cells count: hi is the double sum of the two p (2^-53 of it), lo_sum the float sum of the two lo (u of
|lo0| + |lo1| <= 2^-22 (1 + 2^-19) (|ref0| + |ref1|): 2^-46 of the pair's sum); the bounds of the two cells add.  A dropped cell (skip bit
set) contributes exactly +0.0 in every form."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import terms_ref
from conftest import ARTIFACTS          # where tests leave what they record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 18
OMEGA = 1.7
FORMS = ("double", "float", "compensated", "compensated_fused", "double_fused")       # the probe's order
FUSED_FORM = {"double": False, "float": False, "compensated": False, "compensated_fused": True, "double_fused": True}

B_FLOAT = (2.0 ** -23 + 2.0 ** -24) * (1 + 2.0 ** -20)
U32 = 2.0 ** -24
B_COMP = 5.125 * 2.0 ** -46 * (1 + 2.0 ** -18) + 2.0 ** -51
PAIR_LO = 2.0 ** -46 * (1 + 2.0 ** -18)          # the float sum of a pair's two lo parts, relative to the pair's sum
FLOAT_ROOT_OF_A_DENORMAL_IS_ZERO = True          # v_sqrt_f32 / v_rsq_f32 flush a denormal argument: sqrt -> 0, rsq -> inf (measured, pinned)
MIN_NORMAL = 2.0 ** -126


def comp_abs(msq, rinv):
    """A of the module docstring: what underflow adds to the compensated term's error, float denormals kept."""
    with np.errstate(all="ignore"):
        return 2.0 ** -151 * (1 + 2.0 ** -21) * np.abs(rinv.astype(np.float64)) / np.sqrt(msq.astype(np.float64)) + 2.0 ** -149


def _bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _rest(density):
    d = np.asarray(density, np.float32)
    return np.stack([d * np.float32(4.0 / 9.0)] + [d / np.float32(9.0)] * 4 + [d / np.float32(36.0)] * 4, axis=-1).astype(np.float32)


def _class_l(rng):
    return (rng.random((N, 9, 2), dtype=np.float32) * np.float32(0.02) + np.float32(0.004)).astype(np.float32)


def _momentum_cells(rng, density, em, shape):
    """Cells whose only populations are t[0] = density and one or two of t[1..4]: rho = density + |mx| + |my| rounded, mx = +-t[1 or 3] and
    my = +-t[2 or 4] exactly, the momentum's length 2^em times a factor from [1, 2), its direction random."""
    mag = np.ldexp(rng.uniform(1.0, 2.0, shape), em)
    theta = rng.uniform(0.0, 2.0 * np.pi, shape)
    mx, my = (mag * np.cos(theta)).astype(np.float32), (mag * np.sin(theta)).astype(np.float32)
    pops = np.zeros(shape + (9,), np.float32)
    pops[..., 0] = density
    pops[..., 1] = np.where(mx > 0, mx, 0)
    pops[..., 3] = np.where(mx < 0, -mx, 0)
    pops[..., 2] = np.where(my > 0, my, 0)
    pops[..., 4] = np.where(my < 0, -my, 0)
    return pops


def _class_s(rng):
    """Slow sweeps: density 0.1 - 10 (log-uniform), momentum 2^-10 down to 2^-75 (msq from 2^-20 down through every binade to 2^-149 and to
    0), the two cells of a pair in different binades."""
    i = np.arange(N) // 3                  # the skip code of pair i is i % 3: every binade meets every code
    em = np.stack([-10 - i % 66, -10 - (i * 7 + 13) % 66], axis=-1)
    density = (10.0 ** rng.uniform(-1.0, 1.0, (N, 2))).astype(np.float32)
    return np.moveaxis(_momentum_cells(rng, density, em, (N, 2)), 1, 2)          # (N, 2, 9) -> (N, 9, 2)


def _class_z(rng):
    """Rest and cancelling momenta.  Kinds: 0 only t[0]; 1 t[1] = t[3], t[2] = t[4] (mx = my = 0 exactly); 2 the rest equilibrium of a
    density (the moments cancel up to roundings); 3 mx = my; 4 mx = -my; 5 my = 0; 6 mx = 0 — 3..6 with |m| from 2^-70 to 2^-4."""
    kind = np.arange(N * 2).reshape(N, 2) % 7
    density = (10.0 ** rng.uniform(-1.0, 1.0, (N, 2))).astype(np.float32)
    a = np.ldexp(rng.uniform(1.0, 2.0, (N, 2)), rng.integers(-70, -3, (N, 2))).astype(np.float32)
    pops = np.zeros((N, 2, 9), np.float32)
    pops[..., 0] = density
    sym = kind == 1
    for k in (1, 3):
        pops[..., k] = np.where(sym, density / np.float32(9.0), pops[..., k])
    for k in (2, 4):
        pops[..., k] = np.where(sym, density / np.float32(7.0), pops[..., k])
    pops = np.where((kind == 2)[..., None], _rest(density), pops)
    pops[..., 1] = np.where((kind == 3) | (kind == 4) | (kind == 5), a, pops[..., 1])
    pops[..., 2] = np.where((kind == 3) | (kind == 6), a, pops[..., 2])
    pops[..., 4] = np.where(kind == 4, a, pops[..., 4])
    return np.moveaxis(pops, 1, 2)


def _class_h(rng):
    """Large and special values, a kind per cell: 0 huge momenta (msq up to overflow: inf) beside a huge density; 1 every population zero
    (rho = 0, msq = 0); 2 rho = 0 exactly with a momentum; 3 a denormal density, with and without a denormal momentum; 4 rho in
    [2^126, 2^128): rinv a denormal number or the smallest normal one; 5 a NaN or an infinity among the populations; 6 lattice-like;
    7 a negative density."""
    kind = rng.integers(0, 8, (N, 2))
    one = rng.uniform(1.0, 2.0, (N, 2))
    pops = np.zeros((N, 2, 9), np.float32)
    lattice = np.moveaxis(_class_l(rng), 1, 2)
    with np.errstate(all="ignore"):
        k0 = kind == 0
        pops[..., 0] = np.where(k0, np.ldexp(one, rng.integers(100, 127, (N, 2))), 0).astype(np.float32)
        pops[..., 1] = np.where(k0, np.ldexp(rng.uniform(1.0, 2.0, (N, 2)), rng.integers(40, 127, (N, 2))), 0).astype(np.float32)
        pops[..., 2] = np.where(k0 & (rng.random((N, 2)) < 0.5), pops[..., 1] * np.float32(0.75), 0)
        k2 = kind == 2
        a = np.ldexp(one, rng.integers(-30, 30, (N, 2))).astype(np.float32)
        pops[..., 0] = np.where(k2, -a, pops[..., 0])
        pops[..., 1] = np.where(k2, a, pops[..., 1])
        k3 = kind == 3
        den = rng.integers(1, 1 << 23, (N, 2)).astype(np.uint32).view(np.float32)         # every denormal float
        pops[..., 0] = np.where(k3, den, pops[..., 0])
        pops[..., 2] = np.where(k3 & (rng.random((N, 2)) < 0.5), den, pops[..., 2])
        k4 = kind == 4
        pops[..., 0] = np.where(k4, np.ldexp(one, rng.integers(126, 128, (N, 2))).astype(np.float32), pops[..., 0])
        pops[..., 1] = np.where(k4, np.ldexp(rng.uniform(1.0, 2.0, (N, 2)), rng.integers(-60, 60, (N, 2))).astype(np.float32), pops[..., 1])
        k7 = kind == 7
        pops[..., 0] = np.where(k7, np.float32(-1.0), pops[..., 0])
        pops[..., 1] = np.where(k7, np.float32(0.25), pops[..., 1])
    pops = np.where(((kind == 6) | (kind == 5))[..., None], lattice, pops)
    special = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, (N, 2))]
    where = rng.integers(0, 9, (N, 2))
    for k in range(9):
        pops[..., k] = np.where((kind == 5) & (where == k), special, pops[..., k])
    return np.moveaxis(pops, 1, 2)


# name: (generator, seed, mbits of pair i, skip of pair i)
_I = np.arange(N)
CLASSES = {
    "L": (_class_l, 201, np.zeros(N, np.uint8), (_I % 3).astype(np.uint8)),
    "S": (_class_s, 202, np.zeros(N, np.uint8), (_I % 3).astype(np.uint8)),
    "Z": (_class_z, 203, np.zeros(N, np.uint8), (_I % 3).astype(np.uint8)),
    "H": (_class_h, 204, np.zeros(N, np.uint8), (_I % 3).astype(np.uint8)),
    "K": (_class_l, 205, (_I & 3).astype(np.uint8), ((_I >> 2) & 3).astype(np.uint8)),
}

_cache = {}


def _class(name):
    """pops (N, 9, 2), mbits, skip, and per arithmetic (False: exact, True: fused) the reference's msq, rinv (N, 2) float32 and term (N, 2)
    float64.  Once per process, read-only."""
    if name not in _cache:
        gen, seed, mbits, skip = CLASSES[name]
        pops = np.ascontiguousarray(gen(np.random.default_rng(seed)), np.float32)
        assert pops.shape == (N, 9, 2)
        cells = np.ascontiguousarray(np.moveaxis(pops, 1, 2))                       # (N, 2, 9)
        ref = {}
        for fused in (False, True):
            term, msq, rinv = terms_ref.cell_terms(cells, fused)
            ref[fused] = (msq, rinv, term)
        for a in (pops, mbits, skip) + ref[False] + ref[True]:
            a.setflags(write=False)
        _cache[name] = (pops, mbits, skip, ref)
    return _cache[name]


def _binade(x):
    """floor(log2 x) for finite x > 0, denormals included."""
    m, e = np.frexp(x.astype(np.float64))
    return e.astype(np.int64) - 1


def test_classes_reach_what_they_are_for():
    """From the reference alone: each class lands where it is meant to land.  Printed, then asserted."""
    share = {}
    msq, rinv, term = _class("L")[3][False]
    share["L: cells with a normal term between 1e-3 and 1"] = (float(np.mean((term > 1e-3) & (term < 1.0))), ">=", 0.95)
    msq, rinv, term = _class("S")[3][False]
    pos = msq > 0
    hits = np.bincount(_binade(msq[pos]) + 149, minlength=130)[:130]                # binades 2^-149 .. 2^-20
    share["S: fewest cells in a binade of msq from 2^-149 to 2^-21"] = (float(hits[:129].min()), ">=", 500.0)
    skip = _class("S")[2]
    alone = np.concatenate([msq[skip == 2, 0], msq[skip == 1, 1]])          # cells that are the only counted one of their pair
    hits = np.bincount(_binade(alone[alone > 0]) + 149, minlength=130)[:129]
    share["S: fewest cells counted alone in a binade of msq from 2^-149 to 2^-21"] = (float(hits.min()), ">=", 150.0)
    share["S: cells with msq == 0"] = (float(np.sum(msq == 0)), ">=", 100.0)
    share["S: pairs whose cells' msq lie in different binades"] = (float(np.mean(_binade(np.maximum(msq[:, 0], 1e-45)) != _binade(np.maximum(msq[:, 1], 1e-45)))), ">=", 0.9)
    share["S: smallest 1 / rho"] = (float(rinv.min()), ">=", 0.09)
    share["S: largest 1 / rho"] = (float(rinv.max()), "<=", 10.1)
    msq, rinv, term = _class("Z")[3][False]
    share["Z: cells with msq == 0"] = (float(np.mean(msq == 0)), ">=", 0.25)
    share["Z: cells with msq > 0"] = (float(np.mean(msq > 0)), ">=", 0.5)
    msq, rinv, term = _class("H")[3][False]
    share["H: cells with msq == inf"] = (float(np.sum(np.isinf(msq))), ">=", 1000.0)
    share["H: cells with finite msq >= 2^100"] = (float(np.sum(np.isfinite(msq) & (msq >= 2.0 ** 100))), ">=", 1000.0)
    share["H: cells with 1 / rho infinite"] = (float(np.sum(np.isinf(rinv))), ">=", 1000.0)
    share["H: cells with 1 / rho finite and above 2^126"] = (float(np.sum(np.isfinite(rinv) & (np.abs(rinv) > 2.0 ** 126))), ">=", 100.0)
    share["H: cells with 1 / rho a non-zero denormal"] = (float(np.sum((rinv != 0) & (np.abs(rinv) < MIN_NORMAL))), ">=", 1000.0)
    share["H: cells with a NaN term"] = (float(np.sum(np.isnan(term))), ">=", 1000.0)
    share["H: cells with a negative term"] = (float(np.sum(term < 0)), ">=", 1000.0)
    pops, mbits, skip, ref = _class("K")
    share["K: fewest pairs of one (mbits, skip) code"] = (float(np.bincount(mbits.astype(int) * 4 + skip, minlength=16).min()), ">=", N / 16)
    for what, (value, op, limit) in share.items():
        print(f"  {what}: {value:.6g} (asserted {op} {limit:g})")
    for what, (value, op, limit) in share.items():
        assert {"<=": value <= limit, ">=": value >= limit}[op], (what, value, op, limit)


PROBE_SRC = os.path.join(ROOT, "scripts", "experiments", "terms_probe.hip")


def probe_flags():
    """The flags the library is compiled with, from the build itself (build.py: --offload-arch=gfx950 and COMMON); the module is taken
    from sys.modules, where the package's own import left it (tests/test_f64_cells.py probe_flags)."""
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
    subprocess.run([hipcc, *probe_flags(), PROBE_SRC, "-o", str(tmp_path / "terms_probe")], check=True, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def probed(tmp_path_factory):
    """Compile the probe, write every class, run them all in ONE fresh child process under a timeout.  Returns name -> dict with
    "kept" (float denormals kept), "term" / "lo" per form (N,), and the (N, 2) float planes."""
    tmp = tmp_path_factory.mktemp("terms")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp / "terms_probe")
    subprocess.run([hipcc, *probe_flags(), PROBE_SRC, "-o", exe], check=True, capture_output=True, timeout=300)
    args = []
    for name in CLASSES:
        pops, mbits, skip, _ = _class(name)
        with open(tmp / f"{name}.in", "wb") as fh:
            fh.write(np.uint64(N).tobytes() + np.array([OMEGA, 0.0], np.float32).tobytes())
            fh.write(pops.tobytes() + mbits.tobytes() + skip.tobytes())
        args += [str(tmp / f"{name}.in"), str(tmp / f"{name}.out")]
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    planes = ("msq", "rinv", "msq_fused", "rinv_fused", "raw_sqrt", "raw_rsq")
    for name in CLASSES:
        raw = np.fromfile(tmp / f"{name}.out", np.uint8)
        assert raw.size == 8 + N * (len(FORMS) * 12 + len(planes) * 8)
        d = {"kept": bool(raw[:4].view(np.uint32)[0])}
        term = raw[8:8 + len(FORMS) * N * 8].view(np.float64).reshape(len(FORMS), N)
        off = 8 + len(FORMS) * N * 8
        lo = raw[off:off + len(FORMS) * N * 4].view(np.float32).reshape(len(FORMS), N)
        off += len(FORMS) * N * 4
        fl = raw[off:].view(np.float32).reshape(len(planes), N, 2)
        d["term"] = dict(zip(FORMS, term))
        d["lo"] = dict(zip(FORMS, lo))
        d.update(zip(planes, fl))
        got[name] = d
    return got


def _same_numbers(what, ref, got, bits):
    nan_ref, nan_got = np.isnan(ref), np.isnan(got)
    wrong_nan = np.argwhere(nan_ref != nan_got)
    differ = np.argwhere(~nan_ref & ~nan_got & (bits(ref) != bits(got)))
    print(f"  {what}: {int(nan_ref.sum())} of {ref.size} NaN in the reference; {len(wrong_nan)} NaNs misplaced, {len(differ)} numbers differ")
    for idx in list(wrong_nan[:3]) + list(differ[:3]):
        print(f"    at {tuple(idx)}: reference {ref[tuple(idx)]!r}, device {got[tuple(idx)]!r}")
    assert len(wrong_nan) == 0 and len(differ) == 0, what


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CLASSES))
def test_msq_and_rinv_are_the_restatements(probed, name):
    ref = _class(name)[3]
    got = probed[name]
    assert got["kept"], "the library's flags keep float denormals: every low-range bound of this module is worded for that"
    _same_numbers(f"{name} msq", ref[False][0], got["msq"], _bits32)
    _same_numbers(f"{name} rinv", ref[False][1], got["rinv"], _bits32)
    _same_numbers(f"{name} fused msq", ref[True][0], got["msq_fused"], _bits32)
    _same_numbers(f"{name} fused rinv", ref[True][1], got["rinv_fused"], _bits32)


def _counted(skip):
    """(N, 2) bool: cell j of the pair enters the term."""
    return np.stack([(skip & 1) == 0, (skip & 2) == 0], axis=-1)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["double", "double_fused"])
@pytest.mark.parametrize("name", list(CLASSES))
def test_double_form_is_the_reference_bit_for_bit(probed, name, form):
    pops, mbits, skip, ref = _class(name)
    msq, rinv, term = ref[FUSED_FORM[form]]
    on = _counted(skip)
    with np.errstate(all="ignore"):
        expect = np.where(on[:, 0], term[:, 0], 0.0) + np.where(on[:, 1], term[:, 1], 0.0)
    _same_numbers(f"{name} {form} term", expect, probed[name]["term"][form], _bits64)
    assert np.all(_bits32(probed[name]["lo"][form]) == 0), "the double form leaves lo_sum alone"
    dropped = skip == 3
    assert np.all(_bits64(probed[name]["term"][form][dropped]) == 0), "a dropped pair contributes exactly +0.0"


def _float_ref(msq, term):
    """The float form's own reference per cell: the double term; 0 where msq is a denormal number (the instruction flushes it)."""
    assert FLOAT_ROOT_OF_A_DENORMAL_IS_ZERO
    return np.where((msq > 0) & (msq < MIN_NORMAL), 0.0, term)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["L", "S", "Z", "K"])
def test_float_form_within_one_root_and_one_product(probed, name):
    """Every pair whose counted cells have msq == 0, a denormal msq, or msq >= 2^-126 with a normal rinv and a term between 2^-125 and 2^126
    (all of L, S, Z, K).  |tf - ref| <= B_FLOAT ref per counted cell, + u of the pair's sum where both count (the float addition)."""
    pops, mbits, skip, ref = _class(name)
    msq, rinv, term = ref[False]
    assert np.all(np.isfinite(term)) and np.all((term == 0) | ((term >= 2.0 ** -125) & (term <= 2.0 ** 126))) and np.all(np.abs(rinv) >= MIN_NORMAL)
    on = _counted(skip)
    fref = np.where(on, _float_ref(msq, term), 0.0)
    expect = fref.sum(axis=1)
    bound = B_FLOAT * expect + np.where(on.all(axis=1), U32 * (1 + 2.0 ** -20) * expect, 0.0)
    got = probed[name]["term"]["float"]
    err = np.abs(got - expect)
    rel = np.max(err[expect > 0] / expect[expect > 0]) if np.any(expect > 0) else 0.0
    print(f"  {name} float form: largest |tf - ref| / ref = 2^{np.log2(max(rel, 1e-300)):.2f} (bound 2^{np.log2(B_FLOAT + U32):.2f} for a pair, 2^{np.log2(B_FLOAT):.2f} for a cell)")
    assert np.all(err <= bound), (name, int(np.argmax(err - bound)))
    assert np.all(_bits64(got[expect == 0]) == 0), "cells at rest, cells with a denormal msq and dropped cells contribute exactly +0.0"
    # the raw instructions on a denormal msq, pinned: the root is +0, the reciprocal root +inf (the argument is flushed to zero)
    den = (msq > 0) & (msq < MIN_NORMAL)
    assert np.all(_bits32(probed[name]["raw_sqrt"][den]) == 0) and np.all(np.isposinf(probed[name]["raw_rsq"][den]))
    assert np.all(_bits32(probed[name]["lo"]["float"]) == 0)


def _comp_interval(msq, rinv, term, on):
    """Per pair: the interval the compensated hi + lo must lie in, and which pairs the bounds cover.  Per counted cell:
    msq == 0, rinv finite: [0, 0]; 0 < msq < 2^-126, rinv > 0 normal: [0, ref (1 + 2^-23)]; msq >= 2^-126 finite, rinv normal,
    2^-125 <= |ref| <= 2^126: ref -+ (B_COMP |ref| + A).  Anything else: the pair is not covered."""
    with np.errstate(all="ignore"):
        aref = np.abs(term)
        rest = (msq == 0) & np.isfinite(rinv)
        normal_rinv = np.isfinite(rinv) & (np.abs(rinv) >= MIN_NORMAL)
        low = (msq > 0) & (msq < MIN_NORMAL) & normal_rinv & (rinv > 0)
        main = np.isfinite(msq) & (msq >= MIN_NORMAL) & normal_rinv & (aref >= 2.0 ** -125) & (aref <= 2.0 ** 126)
        b = np.where(main, B_COMP * aref + comp_abs(np.where(main, msq, np.float32(1)), np.where(main, rinv, np.float32(1))), 0.0)
        lo = np.where(rest, 0.0, np.where(low, 0.0, np.where(main, term - b, np.nan)))
        hi = np.where(rest, 0.0, np.where(low, term * (1 + 2.0 ** -23), np.where(main, term + b, np.nan)))
    covered = np.all(~on | rest | low | main, axis=1)
    lo, hi = np.where(on, lo, 0.0), np.where(on, hi, 0.0)
    mag = np.where(on & (low | main), aref, 0.0).sum(axis=1)
    both = on.all(axis=1)
    slack = np.where(both, (PAIR_LO + 2.0 ** -53) * mag, 0.0)
    return lo.sum(axis=1) - slack, hi.sum(axis=1) + slack, covered, rest, low, main


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["compensated", "compensated_fused"])
@pytest.mark.parametrize("name", list(CLASSES))
def test_compensated_form_within_its_derived_bounds(probed, name, form):
    """hi + lo of every covered pair inside the interval of the module docstring; msq == 0 gives exactly 0, msq == inf NaN; a dropped
    cell contributes exactly +0.0 to both parts."""
    pops, mbits, skip, ref = _class(name)
    msq, rinv, term = ref[FUSED_FORM[form]]
    on = _counted(skip)
    lo_b, hi_b, covered, rest, low, main = _comp_interval(msq, rinv, term, on)
    hi_part, lo_part = probed[name]["term"][form], probed[name]["lo"][form]
    got = hi_part + lo_part.astype(np.float64)
    if name in ("L", "S", "Z", "K"):
        assert covered.all(), "every pair of this class lies where a bound is stated"
    assert covered.mean() > 0.2
    ok = (got >= lo_b) & (got <= hi_b)
    bad = covered & ~ok
    print(f"  {name} {form}: {int(covered.sum())} pairs covered, {int(bad.sum())} outside their interval")
    for i in np.flatnonzero(bad)[:5]:
        print(f"    pair {i}: skip {skip[i]} msq {msq[i]} rinv {rinv[i]} ref {term[i]} hi {hi_part[i]!r} lo {lo_part[i]!r} interval [{lo_b[i]!r}, {hi_b[i]!r}]")
    assert not bad.any()
    all_rest = np.all(~on | rest, axis=1)
    assert np.all(hi_part[all_rest] == 0) and np.all(lo_part[all_rest] == 0), "msq == 0 (finite rinv) gives exactly 0"
    dropped = skip == 3
    assert np.all(_bits64(hi_part[dropped]) == 0) and np.all(_bits32(lo_part[dropped]) == 0), "a dropped pair contributes exactly +0.0"
    diverged = np.any(on & np.isinf(msq), axis=1)
    assert np.all(np.isnan(got[diverged])), "msq == inf gives NaN (the reference has inf)"


@pytest.mark.gpu
def test_measured_maxima_per_binade(probed):
    """Class S, pairs with ONE counted cell: per binade of msq the largest |form - ref| / ref of the float form and of both compensated
    forms, beside the bound asserted above.  Written to terms_probe.txt in the tests' artifact directory (conftest.ARTIFACTS; kept as profiles/r13/terms_probe.txt).
    Asserted here: above 2^-104 the compensated maxima are below B_COMP + 2^-151 / msq, whatever the binade."""
    pops, mbits, skip, ref = _class("S")
    single = (skip == 1) | (skip == 2)
    j = np.where(skip == 1, 1, 0)                                           # skip bit 0 drops cell 0: cell 1 counts
    lines = [f"float denormals in the build: {'kept' if probed['S']['kept'] else 'flushed'}",
             "class S of tests/test_terms_cells.py, pairs with one counted cell; per binade of msq: cells, largest |term - ref| / ref",
             f"bounds asserted: float form 2^{np.log2(B_FLOAT):.2f}; compensated 2^{np.log2(B_COMP):.2f} + 2^-151 / msq (+ 2^-149 absolute) from 2^-126 up, [0, ref (1 + 2^-23)] below",
             "binade   cells   float        compensated  compensated_fused"]
    rows = {}
    for form in ("float", "compensated", "compensated_fused"):
        msq, rinv, term = ref[FUSED_FORM[form]]
        idx = np.flatnonzero(single & (msq[np.arange(N), j] > 0))
        m, t = msq[idx, j[idx]], term[idx, j[idx]]
        got = probed["S"]["term"][form][idx] + probed["S"]["lo"][form][idx].astype(np.float64)
        rel = np.abs(got - t) / t
        b = _binade(m)
        for e in np.unique(b):
            rows.setdefault(int(e), {})[form] = (int(np.sum(b == e)), float(rel[b == e].max()))
        if form != "float":
            hi = b >= -104
            assert np.all(rel[hi] <= B_COMP + 2.0 ** -151 * (1 + 2.0 ** -21) / m[hi].astype(np.float64) + 2.0 ** -149 / t[hi])
    msq = ref[False][0]
    den = (msq > 0) & (msq < MIN_NORMAL)
    lines.insert(3, f"raw instructions on the {int(den.sum())} denormal msq of the class: v_sqrt_f32 -> {set(np.unique(probed['S']['raw_sqrt'][den]).tolist())}, "
                    f"v_rsq_f32 -> {set(np.unique(probed['S']['raw_rsq'][den]).tolist())}")
    for e in sorted(rows, reverse=True):
        r = rows[e]
        cell = lambda f: f"2^{np.log2(r[f][1]):8.2f}" if f in r and r[f][1] > 0 else ("0".rjust(10) if f in r else "-".rjust(10))
        lines.append(f"2^{e:<5d} {r.get('float', (0, 0))[0]:7d}   {cell('float')}   {cell('compensated')}   {cell('compensated_fused')}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(ARTIFACTS, exist_ok=True)
    with open(os.path.join(ARTIFACTS, "terms_probe.txt"), "w") as fh:
        fh.write(text)
