"""bench.py end to end on a small panel: a plain run times the steps and prints the line with
nothing else measured, ``--full`` adds the per-kernel pass, the CPU baseline and the H2D load, and
``--dump-outputs`` writes exactly what ``solve_step`` returns for the same arguments."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SMALL = ["--rows", "200003", "--levels", "5000,200", "--k", "3", "--vcov", "HC1", "--steps", "3", "--warmup", "1"]


def _run(capsys, extra):
    import bench

    bench.main(SMALL + extra)
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_times_the_steps_and_dumps_the_last_result(capsys, tmp_path):
    import bench
    from leanfe_amd import synth
    from leanfe_amd._lib import Engine

    line = _run(capsys, ["--dump-outputs", str(tmp_path)])
    assert line["steps"] == 3 and len(line["runs_ms_per_step"]) == 3
    assert line["unit"] == "Mrows/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(200003 / line["ms_per_step"] / 1e3, rel=1e-2)
    # nothing beyond the timed steps was measured
    assert line["kernels_ms"] == {} and line["roofline"] is None
    assert line["cpu_baseline"] is None and line["h2d"] is None

    with Engine(0) as eng:
        eng.synth_load(200003, 3, [5000, 200], synth.betas(3), seed=12345)
        want = bench.output_arrays(bench.solve_step(eng, "HC1"))
    got = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert set(got) == set(want) and {"beta", "se", "rss", "n_obs", "iterations", "df_resid"} <= set(got)
    for name, arr in want.items():
        assert got[name].dtype == np.float64
        np.testing.assert_array_equal(got[name], arr, err_msg=name)  # the fit is deterministic


def test_full_run_adds_the_other_measurements(capsys):
    line = _run(capsys, ["--full"])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["kernels_ms"] and all(v[1] >= 1 for v in line["kernels_ms"].values())
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["iterations"] == line["config"]["iterations"]
    assert line["h2d"]["bytes"] > 0
