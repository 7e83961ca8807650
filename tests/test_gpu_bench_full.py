"""bench.py with and without --full: a plain run prints the headline line alone (no CPU leg, no other mode, no instrumented pass),
--full adds every other leg to the same line, and the --no-* options take legs out of a --full run only."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--scale", "12", "--draws", "20000", "--steps", "3", "--warmup", "1"]
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "ms_per_step_median", "n_gpus", "steps", "warmup",
            "scaling", "vs_baseline", "data", "config"}
FULL_ONLY = {"roofline", "kernels", "kernels_ms_sum", "traffic_source", "alt", "alt_node_order", "cpu_baseline", "gatv2", "epoch_ms"}


def _bench(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, capture_output=True, text=True, env=env,
                       timeout=420)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_alone():
    line = _bench([])
    assert set(line) == HEADLINE
    assert line["metric"] == "GAT-layer fwd+bwd edges/sec" and line["unit"] == "edges/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True and line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(line["config"]["edges"] / (line["ms_per_step"] * 1e-3))
    # the options that take legs out of a --full run are accepted and change nothing here
    assert set(_bench(["--no-cpu", "--no-epoch", "--no-v2", "--no-alt"])) == HEADLINE


def test_full_run_adds_every_leg():
    line = _bench(["--full", "--no-dense-cpu"])
    assert set(line) == HEADLINE | FULL_ONLY
    assert line["cpu_baseline"]["value"] > 0 and line["gatv2"]["ms_per_step"] > 0
    assert line["alt"]["ms_per_step"] > 0 and line["alt_node_order"]["ms_per_step"] > 0
    assert sorted(line["epoch_ms"]) == ["cora", "ppi", "pubmed"] and all(v["ms"] > 0 for v in line["epoch_ms"].values())
    assert line["roofline"]["kernel"] in {k["kernel"] for k in line["kernels"]} and line["kernels_ms_sum"] > 0
    trimmed = _bench(["--full", "--no-cpu", "--no-epoch", "--no-v2", "--no-alt"])
    assert set(trimmed) == HEADLINE | {"roofline", "kernels", "kernels_ms_sum", "traffic_source", "alt", "alt_node_order"}
    assert trimmed["alt"] is None and trimmed["alt_node_order"] is None and trimmed["kernels"]
