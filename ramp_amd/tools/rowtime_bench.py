"""What one score evaluation with a timestep per row costs against one with a shared timestep: ramp_score_rows vs ramp_score at
B = 4096 trajectories x 2 rows, H = 48, S = 4, the bench's launch plan (fp16x3, after calibration), energy gradient included.

The two calls alternate in one process after warm-up; each figure is a pair of device events around one call, median and
min .. max of `reps` repetitions.  ramp_score_rows copies its 8192-entry host table to the device before it launches (one blocking
32 KB copy); the events include it.  Appends to profiles/row_time.txt.
usage: python ramp_amd/tools/rowtime_bench.py [reps] [warm] [--out FILE]"""
from __future__ import annotations

import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ramp_amd import _lib, synth  # noqa: E402
from ramp_amd.models import TemporalUnetInference  # noqa: E402
from ramp_amd.spec import make_unet_spec  # noqa: E402
from ramp_amd.unet import load_numpy_state_dict  # noqa: E402

B, N_RP, H, S, T = 4096, 2, 48, 4, 25


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 20
    warm = int(args[1]) if len(args) > 1 else 5
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "row_time.txt")
    m = TemporalUnetInference(n_support_points=H, state_dim=S, max_rows=B * N_RP)
    load_numpy_state_dict(m, synth.make_unet_state_dict(make_unet_spec(S, H)))
    m = m.eval().to("cuda")
    lat = m.encode_scene(torch.from_numpy(synth.make_cloud(6, 64, 2, seed=3)).cuda())
    m.set_scene(torch.cat([lat, torch.zeros_like(lat)]), [0, 1])
    m.prepare_time_table(T)
    x = torch.from_numpy(synth.make_noise((B, H, S), seed=21)).cuda()
    eps = torch.empty((B * N_RP, H, S), device="cuda")
    rows = np.random.default_rng(7).integers(0, T, B * N_RP).astype(np.int32)
    lib, s = _lib.load(), _lib.current_stream()

    def uniform():
        _lib.check(lib.ramp_score(m.ctx(), _lib.ptr(x), B, N_RP, 11, None, _lib.ptr(eps), s), "ramp_score")

    def per_row():
        _lib.check(lib.ramp_score_rows(m.ctx(), _lib.ptr(x), B, N_RP, rows.ctypes.data_as(_lib.c_i32p), None, _lib.ptr(eps), s), "ramp_score_rows")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for _ in range(warm):
        uniform(); per_row()
    mode = m.score_mode()
    tu, tr = [], []
    for _ in range(reps):
        tu.append(timed(uniform)); tr.append(timed(per_row))
    mu, mr = statistics.median(tu), statistics.median(tr)
    lines = [f"one evaluation, B = {B} x {N_RP} rows, H = {H}, S = {S}, {mode}, eps only; {reps} alternating repetitions after {warm} warm-up pairs",
             f"  ramp_score      (one t)      median {mu:8.3f} ms   min {min(tu):8.3f}   max {max(tu):8.3f}",
             f"  ramp_score_rows (t per row)  median {mr:8.3f} ms   min {min(tr):8.3f}   max {max(tr):8.3f}",
             f"  per-row / uniform = {mr / mu:.4f}"]
    print("\n".join(lines))
    with open(out, "a", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
