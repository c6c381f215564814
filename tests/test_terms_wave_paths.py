"""The two paths of the owned pair's sum|u| term in lbm_multi_kernel's tall geometry (kernels/common.h finish_pair_owned).

A wave in which no lane drops a cell from its term takes plain sums; every other wave applies its selects to the float parts.  Both
must give the double finish_pair gives: (double)p.x + (double)p.y + (double)(lo.x + lo.y), a dropped cell contributing +0.

Part 1 runs the shipped function in scripts/experiments/terms_probe.hip (option --owned), one pair per lane, on four waves of the same
cell states: a wave without a dropped cell, a wave whose skip codes cycle 0 1 2 3, a wave with a dropped cell in lane 0 and in lane
63 only, a wave of dropped pairs.  Equal (state, skip) must give equal bits whichever wave the pair sat in, and the opt-in form's
double must be the existing compensated instantiation's hi + (double)lo_sum bit for bit.

Part 2 runs whole five-step launches on 192 x 72 (3 x 3 tiles of 64 x 24; a wave is two tile rows of 32 pairs) with three obstacle
layouts: none (every wave on the plain path), exactly one blocked cell per wave (no wave on it), and tests/test_multi5.py's
position_obstacles (both).  Populations bit for bit against the oracle, the per-step sums within tests/test_terms_sums.py's bound
for the multi family, whose census condition is asserted from the reference alone (and was checked on a CPU for these three decks:
the smallest term of a free cell is above 1e-3 of the mean in every step).

Not compared: the same run on the standard geometry.  Its lanes add the low parts in a float accumulator that is widened once per
launch (k_substeps), the tall geometry adds hi + (double)lo per pair: two summation orders, whose sums need not agree in the last
bit at the parent commit either; tests/test_terms_sums.py holds both to the same reference bound."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import terms_ref
import test_terms_cells as tc
import test_terms_sums as ts
from test_multi5 import position_obstacles
from test_owned_lanes import TX, TY

pytestmark = pytest.mark.gpu

WAVE = 64
OWNED_FORMS = ("owned", "owned_fused", "guarded", "guarded_fused")          # the probe's order in OUT.owned


def _base_states():
    """16 pair states (9, 2): lattice-like ones, slow ones whose msq runs down to the denormal range and below 2^-126, and rest (msq = 0)."""
    rng = np.random.default_rng(77)
    s = np.zeros((16, 2, 9), np.float32)
    s[:8] = (rng.random((8, 2, 9), dtype=np.float32) * np.float32(0.02) + np.float32(0.004))
    density = np.float32(0.75)
    for i, em in enumerate((-20, -40, -55, -62, -64, -70)):             # momentum 2^em: msq = 2^(2 em), from 2^-40 down to 2^-140
        s[8 + i] = tc._momentum_cells(rng, np.full(2, density, np.float32), np.array([em, em - 1]), (2,))
    s[14, :, 0] = density                                                 # at rest: mx = my = 0 exactly
    s[15, 0, 0], s[15, 1] = density, s[3, 1]                              # one cell at rest beside a lattice-like one
    return np.ascontiguousarray(np.moveaxis(s, 1, 2))                     # (16, 9, 2)


def _probe_input():
    base = _base_states()
    states = base[np.arange(WAVE) // 4]                                   # the wave's 64 states: each base state four times in a row
    pops = np.ascontiguousarray(np.concatenate([states] * 4), np.float32)
    lane = np.arange(WAVE)
    skip = np.concatenate([np.zeros(WAVE, np.uint8), (lane % 4).astype(np.uint8),
                           np.where(lane == 0, 1, np.where(lane == WAVE - 1, 2, 0)).astype(np.uint8), np.full(WAVE, 3, np.uint8)])
    mbits = np.concatenate([np.zeros(WAVE, np.uint8), skip[WAVE:2 * WAVE], np.zeros(WAVE, np.uint8), skip[3 * WAVE:]])   # obstacles are dropped cells
    return pops, mbits, skip


@pytest.fixture(scope="module")
def probed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wave_paths")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp / "terms_probe")
    subprocess.run([hipcc, *tc.probe_flags(), tc.PROBE_SRC, "-o", exe], check=True, capture_output=True, timeout=300)
    pops, mbits, skip = _probe_input()
    n = len(skip)
    with open(tmp / "w.in", "wb") as fh:
        fh.write(np.uint64(n).tobytes() + np.array([tc.OMEGA, 0.0], np.float32).tobytes())
        fh.write(pops.tobytes() + mbits.tobytes() + skip.tobytes())
    r = subprocess.run([exe, "--owned", str(tmp / "w.in"), str(tmp / "w.out")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(tmp / "w.out", np.uint8)
    assert raw.size == 8 + n * (len(tc.FORMS) * 12 + 6 * 8), "the probe's own output is what it is without the option"
    term = raw[8:8 + len(tc.FORMS) * n * 8].view(np.float64).reshape(len(tc.FORMS), n)
    off = 8 + len(tc.FORMS) * n * 8
    lo = raw[off:off + len(tc.FORMS) * n * 4].view(np.float32).reshape(len(tc.FORMS), n)
    off += len(tc.FORMS) * n * 4
    msq = raw[off:off + n * 8].view(np.float32).reshape(n, 2)
    owned = np.fromfile(tmp / "w.out.owned", np.float64).reshape(len(OWNED_FORMS), n)
    return {"term": dict(zip(tc.FORMS, term)), "lo": dict(zip(tc.FORMS, lo)), "msq": msq, "owned": dict(zip(OWNED_FORMS, owned)), "skip": skip, "pops": pops}


def _b64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_the_states_reach_the_low_range(probed):
    msq = probed["msq"][:WAVE]
    print(f"  msq of the wave's cells: {int(np.sum(msq == 0))} zero, {int(np.sum((msq > 0) & (msq < 2.0 ** -126)))} below 2^-126, {int(np.sum(msq >= 2.0 ** -126))} normal")
    assert np.sum(msq == 0) >= 4 and np.sum((msq > 0) & (msq < 2.0 ** -126)) >= 8 and np.sum(msq > 2.0 ** -20) >= 32
    assert np.all(np.isfinite(probed["owned"]["owned"]))


@pytest.mark.parametrize("form,existing", [("owned", "compensated"), ("owned_fused", "compensated_fused"), ("guarded", "compensated"), ("guarded_fused", "compensated_fused")])
def test_owned_form_is_the_compensated_instantiation(probed, form, existing):
    """finish_pair_owned's double against finish_pair's from finish_pair_lo's two parts, hi + (double)lo_sum: all 256 pairs, every bit."""
    expect = probed["term"][existing] + probed["lo"][existing].astype(np.float64)
    got = probed["owned"][form]
    differ = np.flatnonzero(_b64(expect) != _b64(got))
    print(f"  {form} against {existing}: {len(differ)} of {len(got)} pairs differ")
    for i in differ[:5]:
        print(f"    pair {i} (skip {probed['skip'][i]}): {expect[i]!r} expected, {got[i]!r}")
    assert len(differ) == 0
    assert np.all(_b64(got[probed["skip"] == 3]) == 0), "a dropped pair contributes exactly +0.0"


@pytest.mark.parametrize("form", OWNED_FORMS + ("compensated", "compensated_fused"))
def test_equal_state_and_skip_give_equal_bits_in_every_wave(probed, form):
    """The plain path (wave 0) against the select path (waves 1 - 3) for skip = 0, and the select path's waves among themselves."""
    skip, pops = probed["skip"], probed["pops"]
    if form in OWNED_FORMS:
        val = _b64(probed["owned"][form])
    else:
        val = _b64(probed["term"][form]) ^ (np.ascontiguousarray(probed["lo"][form]).view(np.uint32).astype(np.uint64) << np.uint64(17))   # both parts
    seen, compared = {}, 0
    for i in range(len(skip)):
        key = (pops[i].tobytes(), int(skip[i]))
        if key in seen:
            compared += 1
            assert val[i] == val[seen[key]], (form, i, seen[key], int(skip[i]))
        else:
            seen[key] = i
    across = sum(1 for i in range(2 * WAVE, 3 * WAVE) if skip[i] == 0)
    print(f"  {form}: {compared} pairs compared with an earlier pair of equal state and skip ({across} of them wave 2's skip = 0 lanes against wave 0)")
    assert compared >= 160 and across == WAVE - 2


def one_per_wave(nx, ny):
    """Exactly one blocked cell per wave of every tile: lane 0's .x in even waves, lane 63's .y in odd waves."""
    obst = np.zeros((ny, nx), np.int32)
    for y0 in range(0, ny, TY):
        for x0 in range(0, nx, TX):
            for w in range(TY // 2):
                if w % 2 == 0:
                    obst[y0 + 2 * w, x0] = 1
                else:
                    obst[y0 + 2 * w + 1, x0 + TX - 1] = 1
    return obst


LAYOUTS = {"none": lambda nx, ny: np.zeros((ny, nx), np.int32), "one_per_wave": one_per_wave, "positions": lambda nx, ny: position_obstacles(nx, ny, 31)}
_refs = {}


def reference(lbm, layout, nx, ny, n):
    if layout not in _refs:
        p = lbm.Params(nx, ny, n, 4, 0.1, 0.005, ts.OMEGA)
        obst = np.ascontiguousarray(LAYOUTS[layout](nx, ny), np.int32)
        cells0 = terms_ref.random_state(ny, nx, 4242)
        _refs[layout] = (p, obst, cells0, terms_ref.StepSums(p, obst, cells0, n))
    return _refs[layout]


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_whole_launches(lbm, monkeypatch, layout):
    monkeypatch.setenv("LBM_TUNE_TILE_MAX", "0")
    monkeypatch.setenv("LBM_TUNE_MULTI_K", "5")
    monkeypatch.setenv("LBM_TUNE_MULTI_GEOM", "2")
    nx, ny, n = 3 * TX, 3 * TY, 10
    p, obst, cells0, ref = reference(lbm, layout, nx, ny, n)
    if layout == "one_per_wave":
        waves = obst.reshape(ny // 2, 2, nx // TX, TX).sum(axis=(1, 3))
        assert np.all(waves == 1)
    sums, kernel, cells = ts.run_whole(lbm, p, obst, cells0, n)
    assert kernel == "lbm_multi_kernel<5>", kernel
    differing = int(np.count_nonzero(ts._bits(cells) != ts._bits(ref.cells)))
    print(f"  {layout}: {int(obst.sum())} blocked cells, {differing} differing population words")
    assert differing == 0
    ts.check(sums, ref, n, "multi", "compensated", f"{kernel} {nx}x{ny} {layout}")
