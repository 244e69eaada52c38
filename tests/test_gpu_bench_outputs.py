"""bench.py --dump-outputs and the plain / --full split on the GPU, through
bench.main() on a small workload (8 games, 64 sims/move, a 128x2b net):

* the dump holds the last timed step's outputs as the caller of the timed path
  receives them: actions, finished, features, policy, float32, the engine's
  shapes; actions are legal action indices (or -1), the target policies sum
  to 1;
* the same arguments give the same arrays (seeded weights, openings, engine);
* --steps sets the number of timed steps: one step less gives other arrays;
* a plain line carries the headline fields and none of the --full sub-records.
"""

import json

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--games", "8", "--sims", "64", "--threads", "2", "--batch", "8", "--history", "2",
         "--channels", "128", "--blocks", "2", "--hidden", "32", "--warmup", "1"]


def _run(capsys, tmp_path, name, steps):
    d = tmp_path / name
    bench.main(SMALL + ["--steps", str(steps), "--dump-outputs", str(d)])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), {p.stem: np.load(p) for p in sorted(d.glob("*.npy"))}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return tmp_path_factory.mktemp("bench_outputs")


def test_dump_outputs_and_plain_line(capsys, runs):
    line, a = _run(capsys, runs, "a", 3)
    _, b = _run(capsys, runs, "b", 3)
    _, c = _run(capsys, runs, "c", 2)
    assert sorted(a) == ["actions", "features", "finished", "policy"]
    assert a["actions"].shape == (8,) and a["finished"].shape == (8,)
    assert a["features"].shape == (8, 8, 5, 8, 8) and a["policy"].shape == (8, 8, 65)
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert np.all((a["actions"] >= -1) & (a["actions"] <= 64) & (a["actions"] == np.round(a["actions"])))
    assert np.all(np.isin(a["finished"], np.arange(8.0)))  # result bits 0-1, unexpanded-root bit 2
    assert np.all(np.isin(a["features"], (0.0, 1.0)))
    # after 4 moves from openings of <= 8 plies every game is still running: targets for all of them
    assert np.all(a["finished"] == 0) and np.all(a["actions"] >= 0)
    np.testing.assert_allclose(a["policy"].sum(-1), 1.0, atol=1e-5)
    for k in a:  # same arguments: the same arrays
        assert np.array_equal(a[k], b[k]), k
    # one timed step less: another move's outputs
    assert not np.array_equal(a["features"], c["features"])
    # the plain line: the headline fields, none of the --full sub-records
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "bf16"
    assert line["unit"] == "simulations/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - 8 * 64 * 3 / (line["ms_per_step"] * 3e-3)) <= 1e-3 * line["value"]
    assert "roofline" in line  # from the timed region's own counters
    for k in ("sustained", "net_outputs", "deep_tree", "other_configs", "latency", "cpu_baseline"):
        assert k not in line, k
