#!/usr/bin/env python3
"""Writes tests/golden/sim3_opt_golden.npz: the four small pairs of tests/sim3_golden_cases.py with the outputs of the analytic model
(tests/sim3_opt_model.py).  Data only; tests/test_gpu_sim3_opt.py compares the device against it without importing the model.
    python tools/gen_sim3_golden.py"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sim3_golden_cases  # noqa: E402
import sim3_opt_model as m  # noqa: E402


def main():
    out = {}
    cases = sim3_golden_cases.cases()
    for k, pb in enumerate(cases):
        r = m.solve(pb)
        rows = np.concatenate([pb["P1c"], pb["P2c"], pb["obs1"], pb["obs2"], pb["w1"][:, None], pb["w2"][:, None]], 1)
        assert np.array_equal(rows.astype(np.float32).astype(np.float64), rows)      # float values widened: stored as float32
        out["rows%d" % k] = rows.astype(np.float32)                                   # [n][12] = P1c P2c obs1 obs2 w1 w2
        kb = pb["cam1"]["kb8"]
        # K (4), kb8 (4, NaN = Pinhole), th2, fix_scale, sim3 in (8), sim3 out (8), n_in, n_corr, n_bad
        out["meta%d" % k] = np.r_[pb["cam1"]["K"], kb if kb is not None else [np.nan] * 4, np.float32(pb["th2"]), float(pb["fix_scale"]),
                                  pb["sim3"], r["sim3"], r["n_in"], r["n_corr"], r["n_bad"]].astype(np.float64)
        out["flag%d" % k] = r["flag"]
        print(k, len(pb["P1c"]), r["n_in"], r["n_corr"], r["n_bad"])
    out["count"] = np.int32(len(cases))
    path = os.path.join(ROOT, "tests", "golden", "sim3_opt_golden.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
