"""bench.py's options: --full is there and off by default, so a run without it measures the headline alone."""
import bench


def test_full_is_an_option_that_is_off_by_default(monkeypatch):
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2"])
    plain = bench.parse()
    assert plain.full is False and (plain.steps, plain.warmup) == (4, 2)
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2", "--full"])
    assert bench.parse().full is True
