#!/usr/bin/env python3
"""The four shipped decks, full length, through `LBM_PRECISION=double bin/d2q9-bgk`, each held to check.py's rule against
tests/golden/check/ (tolerance 1 %) and to the Reynolds number the reference published (tests/golden/f64_published.json), with the
largest relative distance of av_vels from the shipped file beside it.

    python scripts/check_f64_decks.py [--decks 128x128,128x256] [--flags 512] [--ranks 4] [--out profiles/r07/check_f64_decks.txt]

LBM_TUNE_TILE64_MAX and LBM_TUNE_TILE64_GEOM of the caller's environment reach the CLI; every other LBM_* variable is dropped.  Each
deck's report ends with the kernel that ran and its launches (LBM_DESCRIBE=1).

--flags: LBM_FLAGS of the CLI, the lbm64_create flags (512 = LBM64_FLAG_TILE_STEPS, 1024 = LBM64_FLAG_MULTI_STEPS, 1536 = both: several steps per launch where the grid is eligible; 4096 = LBM64_FLAG_MULTI_ANY_SIZE: 1024 on the shipped decks, which 32 x 16 tiles cover).

--ranks N: LBM64_RANKS of the CLI: the deck as N row blocks (include/lbm_d2q9_f64_rows.h), rank r on device r % (device count); then
--flags takes 0, 1 or 2 only.

One CLI process per deck, each under a time limit; the first failure ends the script (exit status 1)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mpilattice_boltzmann_amd as lbm  # noqa: E402

DECKS = ("128x128", "128x256", "256x256", "1024x1024")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decks", default=",".join(DECKS))
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per deck")
    ap.add_argument("--flags", type=int, default=0, help="LBM_FLAGS: lbm64_create flags (512: LBM64_FLAG_TILE_STEPS, 1024: LBM64_FLAG_MULTI_STEPS, 1536: both, 4096: LBM64_FLAG_MULTI_ANY_SIZE)")
    ap.add_argument("--ranks", type=int, default=0, help="LBM64_RANKS: the deck as this many row blocks (0: one context)")
    a = ap.parse_args()
    lbm.build()
    with open(os.path.join(GOLDEN, "f64_published.json")) as fh:
        published = json.load(fh)["reynolds"]
    lines = [f"# LBM_PRECISION=double{f' LBM_FLAGS={a.flags}' if a.flags else ''}{f' LBM64_RANKS={a.ranks}' if a.ranks else ''} bin/d2q9-bgk on the shipped decks (full length), then checker.check_files against tests/golden/check/ (tolerance 1 %)",
             "# and the Reynolds line against the number the reference published"]
    ok = True
    for name in a.decks.split(","):
        env = {k: v for k, v in os.environ.items() if not k.startswith(("LBM_", "LBM64_")) or k in ("LBM_TUNE_TILE64_MAX", "LBM_TUNE_TILE64_GEOM", "LBM_TUNE_MULTI64_K", "LBM_TUNE_MULTI64_MIN")}
        env["LBM_PRECISION"] = "double"
        env["LBM_DESCRIBE"] = "1"                      # one line on stderr: the kernel that ran and its launches
        if a.flags:
            env["LBM_FLAGS"] = str(a.flags)
        if a.ranks:
            env["LBM64_RANKS"] = str(a.ranks)
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [lbm.CLI_PATH, os.path.join(GOLDEN, "decks", f"input_{name}.params"), os.path.join(GOLDEN, "decks", f"obstacles_{name}.dat")]
            r = subprocess.run(cmd, cwd=tmp, env=env, capture_output=True, text=True, timeout=a.timeout)
            lines.append(f"== {name}")
            if r.returncode != 0:
                lines += [f"exit status {r.returncode}", r.stderr.strip()]
                ok = False
                break
            out = r.stdout.splitlines()
            ran = [l for l in r.stderr.splitlines() if l.startswith("kernel: ")]
            if len(ran) != 1:
                lines.append("the CLI did not say which kernel ran")
                ok = False
                break
            ref_fs = os.path.join(GOLDEN, "check", f"{name}.final_state.dat.gz")
            have_fs = os.path.exists(ref_fs)
            ref_av = os.path.join(GOLDEN, "check", f"{name}.av_vels.dat.gz")
            rep = lbm.checker.check_files(ref_av, ref_fs if have_fs else None, os.path.join(tmp, "av_vels.dat"),
                                          os.path.join(tmp, "final_state.dat") if have_fs else None)
            golden, mine = lbm.checker.load_av_vels(ref_av), lbm.checker.load_av_vels(os.path.join(tmp, "av_vels.dat"))
            av_rel = float(np.max(np.abs(mine - golden) / np.abs(golden)))
        re_text = out[1].split("\t")[-1]
        pub = published[name]
        re_rel = abs(float(re_text) - float(pub["value"])) / float(pub["value"])
        report = [rep.message, f"av_vels, largest relative distance from the shipped file: {av_rel:.3e}",
                  f"Reynolds number: {re_text}   published ({pub['source']}): {pub['value']}   relative distance {re_rel:.3e}",
                  out[2], out[5], ran[0]]
        lines += report
        ok = ok and rep.ok
        print("\n".join([f"== {name}"] + report), flush=True)
        if not rep.ok:
            break
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
