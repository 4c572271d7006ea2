"""What K distinct plans per scene cost: ramp_select_diverse_scenes at the two shapes that matter,

  one scene     B = 4096, H = 48, S = 4, D = 2, K in {1, 4, 16}        (the static planner's batch)
  many scenes   64 scenes x 64 rows, the same H, S, D, K in {1, 4, 16}

beside ramp_select_scored_scenes on the same arrays (the single selection every caller gets today) and beside ONE score evaluation at
B = 4096 x 2 rows, H = 48 (rowtime_bench.py's set-up), which is what a sampling job pays per denoising step.  The trajectories are
sinusoidal detours whose amplitudes spread over [-1, 1], so that min_sep = 0.25 leaves about five modes: K = 16 runs out of candidates
and still pays all its passes.  The launch count of a call is 2 K + 1 (K picks, K updates, the counts), whatever the scenes.

Every figure is per call: `launches` back-to-back calls between two device events, `reps` such windows per side after `warm` warm-up
calls, the sides alternating window by window in one process; median and min .. max over the windows.  The score evaluation is timed
one call per window.  Appends to profiles/diverse_select.txt.
usage: python ramp_amd/tools/diverse_bench.py [--reps 15] [--launches 50] [--warm 5] [--no-score] [--out FILE]"""
from __future__ import annotations

import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ramp_amd import _lib  # noqa: E402
from ramp_amd.tools.clearance_bench import make_score, opt, window  # noqa: E402

H, S, D = 48, 4, 2
SHAPES = {"one scene of 4096": [4096], "64 scenes of 64": [64] * 64}
KS = (1, 4, 16)
MIN_SEP = 0.25


def make_inputs(counts):
    B = sum(counts)
    rng = np.random.default_rng(17)
    x = rng.uniform(-1, 1, (B, H, S)).astype(np.float32)
    prof = np.sin(np.pi * (np.arange(H) + 0.5) / H)
    x[:, :, 0] = np.linspace(-1, 1, H)[None, :] + rng.uniform(-0.02, 0.02, (B, H))
    x[:, :, 1] = rng.uniform(-1, 1, B)[:, None] * prof[None, :] + rng.uniform(-0.02, 0.02, (B, H))
    keep = dict(t=torch.from_numpy(x).cuda(), first=torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).cuda(),
                mask=torch.from_numpy((rng.random(B) < 0.3).astype(np.int32)).cuda(),
                plen=torch.from_numpy(rng.uniform(1, 9, B).astype(np.float32)).cuda(),
                smooth=torch.from_numpy(rng.uniform(2, 34, B).astype(np.float32)).cuda())
    return B, len(counts), keep


def make_diverse(counts, K):
    B, n, keep = make_inputs(counts)
    out = dict(best=torch.empty(n, K, H, S, device="cuda"), rows=torch.empty(n, K, dtype=torch.int32, device="cuda"),
               res=torch.empty(n, 4, dtype=torch.int32, device="cuda"), mode=torch.empty(B, dtype=torch.int32, device="cuda"),
               sep=torch.empty(B, device="cuda"), count=torch.empty(n, K, dtype=torch.int32, device="cuda"),
               scratch=torch.empty(2 * B + n, dtype=torch.int32, device="cuda"))
    lib, s = _lib.load(), _lib.current_stream()

    def launch():
        _lib.check(lib.ramp_select_diverse_scenes(
            keep["t"].data_ptr(), B, H, S, D, keep["first"].data_ptr(), n, keep["mask"].data_ptr(), keep["plen"].data_ptr(),
            keep["smooth"].data_ptr(), 0.1, 0.9, K, MIN_SEP, 0, out["best"].data_ptr(), out["rows"].data_ptr(), out["res"].data_ptr(),
            out["mode"].data_ptr(), out["sep"].data_ptr(), out["count"].data_ptr(), out["scratch"].data_ptr(), s), "ramp_select_diverse_scenes")
    launch.keep, launch.out = keep, out
    return launch


def make_single(counts):
    B, n, keep = make_inputs(counts)
    best, res = torch.empty(n, H, S, device="cuda"), torch.empty(n, 4, dtype=torch.int32, device="cuda")
    lib, s = _lib.load(), _lib.current_stream()

    def launch():
        _lib.check(lib.ramp_select_scored_scenes(keep["t"].data_ptr(), B, H, S, keep["first"].data_ptr(), n, keep["mask"].data_ptr(),
                                                 keep["plen"].data_ptr(), keep["smooth"].data_ptr(), 0.1, 0.9, best.data_ptr(), res.data_ptr(), s),
                   "ramp_select_scored_scenes")
    launch.keep = (keep, best, res)
    return launch


def main():
    reps, launches, warm = int(opt("--reps", "15")), int(opt("--launches", "50")), int(opt("--warm", "5"))
    out = opt("--out", os.path.join(ROOT, "profiles", "diverse_select.txt"))
    sides, found = [], {}
    for name, counts in SHAPES.items():
        sides.append((f"{name}: ramp_select_scored_scenes (1 launch)", make_single(counts), launches))
        for K in KS:
            fn = make_diverse(counts, K)
            sides.append((f"{name}: ramp_select_diverse_scenes K = {K:2d} ({2 * K + 1} launches)", fn, launches))
            found[(name, K)] = fn
    if "--no-score" not in sys.argv:
        sides.append((f"one score evaluation, B = 4096 x 2 rows, H = {H}, S = {S}", make_score(), 1))
    for _, fn, _n in sides:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    got = {name: [] for name, _, _ in sides}
    for _ in range(reps):
        for name, fn, n in sides:
            got[name].append(window(fn, n))
    lines = [f"# diverse_bench: H = {H}, S = {S}, D = {D}, min_sep = {MIN_SEP} (mean metric); ms per call, {launches} calls per window between "
             f"device events, {reps} alternating windows after {warm} warm-up calls (score: one call per window)"]
    med = {}
    for name, _, _ in sides:
        v = got[name]
        med[name] = statistics.median(v)
        lines.append(f"  {name:80s} median {med[name]:9.4f} ms   min {min(v):9.4f}   max {max(v):9.4f}")
    names = [n for n, _, _ in sides]
    score = next((n for n in names if n.startswith("one score")), None)
    for shape in SHAPES:
        single = next(n for n in names if n.startswith(shape) and "scored" in n)
        for K in KS:
            dv = next(n for n in names if n.startswith(shape) and f"K = {K:2d} " in n)
            sel = found[(shape, K)].out["res"][:, 1].float().mean().item()
            line = f"  {shape}, K = {K:2d}: {2 * K + 1} launches, {sel:.1f} selected per scene, / single selection = {med[dv] / med[single]:.2f}"
            if score:
                line += f", / one score evaluation = {med[dv] / med[score]:.4f}, share of a 25-step job = {100 * med[dv] / (25 * med[score]):.3f} %"
            lines.append(line)
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
