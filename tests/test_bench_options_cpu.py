"""bench.py's options without a GPU: a plain run carries only what its headline figure needs, --full adds the other legs at
their default budgets, and a budget given on the command line holds either way."""
import bench


def _legs(a):
    return a.cpu_seconds, a.fit_iters, a.long_seconds, a.weak_steps


def test_plain_run_runs_no_extra_leg():
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not a.full and _legs(a) == (0.0, 0, 0.0, 0)
    assert a.steps == 20 and a.warmup == 5 and a.config == 3 and not a.no_kernel_timing


def test_full_runs_every_leg_at_its_default_budget():
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert a.full and _legs(a) == (30.0, 100, 2.0, 20)
    assert a.steps == 20 and a.warmup == 5 and not a.no_other_configs


def test_explicit_budgets_hold_with_and_without_full():
    a = bench.parse_args(["--cpu-seconds", "2", "--fit-iters", "3", "--weak-steps", "2", "--long-seconds", "1"])
    assert not a.full and _legs(a) == (2.0, 3, 1.0, 2)
    a = bench.parse_args(["--full", "--cpu-seconds", "0", "--fit-iters", "0", "--weak-steps", "0", "--long-seconds", "0"])
    assert a.full and _legs(a) == (0.0, 0, 0.0, 0)
    a = bench.parse_args(["--full", "--cpu-iters", "0"])  # (the older way to turn the CPU oracle off)
    assert a.cpu_seconds == 0.0 and a.fit_iters == 100


def test_default_steps_follow_the_config():
    assert bench.parse_args([]).steps == 2000
    assert bench.parse_args(["--config", "2"]).steps == 100
    assert bench.parse_args(["--config", "5"]).steps == 10
