"""CPU: reward_comparison.py's host side -- the result dictionary from synthetic TrainingLog
tables, the window rule against a literal restatement of the reference's loop
(training/reward_comparison.py:113-124), the report, the JSON and the command lines."""
import json
import math

import numpy as np
import pytest

from dexterous_rl_manipulation_amd import reward_comparison as RC
from dexterous_rl_manipulation_amd import train
from dexterous_rl_manipulation_amd.training_run import COLS, COLUMNS, TrainingLog

NAN = float("nan")
IDX = {name: k for k, name in enumerate(COLUMNS)}


def reference_window_rule(values, window, threshold):
    """The reference's loop, literally: values are appended one at a time; at the first length
    >= window whose last `window` entries average above the threshold, the step is
    index - window + 1."""
    seen, step = [], None
    for index, v in enumerate(values):
        seen.append(v)
        if step is None and len(seen) >= window:
            recent_avg = np.mean(seen[-window:])
            if recent_avg > threshold:
                step = index - window + 1
    return step


def make_log(returns, rates=None, lengths=None, episodes=None, step_rewards=None, window=10, threshold=0.5, first=0):
    """A TrainingLog as fit(converge=("mean_return", window, threshold)) would leave it."""
    rows = len(returns)
    rates = [0.0] * rows if rates is None else rates
    table = np.zeros((rows, COLS))
    table[:, IDX["iteration"]] = np.arange(first, first + rows)
    table[:, IDX["mean_return"]] = returns
    table[:, IDX["success_rate"]] = rates
    table[:, IDX["mean_length"]] = [7.0] * rows if lengths is None else lengths
    table[:, IDX["episodes"]] = [0.0 if math.isnan(r) else 5.0 for r in returns] if episodes is None else episodes
    table[:, IDX["mean_step_reward"]] = [0.0] * rows if step_rewards is None else step_rewards
    first_row = reference_window_rule(returns, window, threshold)
    converged_row = -1 if first_row is None else first_row + window - 1  # the header keeps the window's LAST row
    header = {"rows_written": rows, "best_row": -1, "converged_row": converged_row, "best_score": -math.inf}
    return TrainingLog(table, header, window, {"converge": ["mean_return", window, threshold]})


CROSSING = [0.0, 0.2, 0.9, 0.9, 0.9, 0.1, 0.9]


@pytest.mark.parametrize("values,window,threshold,want", [
    ([0.9, 0.9], 3, 0.5, None),                # fewer rows than the window
    ([0.6, 0.6, 0.6, 0.0], 3, 0.5, 0),         # the first full window crosses
    ([0.0, 0.6, 0.6, 0.6, 0.6], 3, 0.5, 1),    # a later one
    ([0.5, 0.5, 0.5, 0.5], 2, 0.5, None),      # equal to the threshold is not above it
    ([0.1, 0.2, 0.3, 0.2], 2, 0.5, None),      # no crossing
    ([0.9, NAN, 0.9, 0.9, 0.9], 2, 0.5, 2),    # a window holding a NaN does not qualify
    (CROSSING, 3, 0.5, 1),
])
def test_window_rule_is_the_references(values, window, threshold, want):
    assert reference_window_rule(values, window, threshold) == want
    assert RC.window_convergence(values, window, threshold) == want
    # on both columns of the dictionary: the log's own rule for the return, the host's for the rate
    out = RC.comparison_from_log(make_log(values, rates=values, window=window, threshold=threshold, first=4), "sparse",
                                 threshold, window)
    shifted = None if want is None else 4 + want  # steps are iteration values: this log starts at iteration 4
    assert out["convergence_step"] == shifted and out["success_convergence_step"] == shifted


def test_success_convergence_is_independent_of_the_return_rule():
    returns = [-0.1] * 12                     # a sparse arm: the return never crosses 0.5 ...
    rates = [0.0] * 5 + [0.8] * 7            # ... while the success rate does, in its third window
    out = RC.comparison_from_log(make_log(returns, rates), "sparse")
    assert out["convergence_step"] is None
    assert out["success_convergence_step"] == reference_window_rule(rates, 10, 0.5) == 2


def test_dictionary_keys_and_series():
    returns, rates, lengths = [1.0, 2.0, 4.0], [0.25, 0.5, 0.75], [9.0, 8.0, 7.0]
    log = make_log(returns, rates, lengths, step_rewards=[0.1, 0.2, 0.3])
    out = RC.comparison_from_log(log, "dense")
    assert set(out) == {"episode_rewards", "episode_steps", "success_rates", "convergence_step", "mean_reward",
                        "std_reward", "final_success_rate", "log", "success_convergence_step", "mean_step_rewards",
                        "reward_type"}
    assert out["episode_rewards"] == returns and out["episode_steps"] == lengths and out["success_rates"] == rates
    assert out["mean_step_rewards"] == [0.1, 0.2, 0.3] and out["log"] is log and out["reward_type"] == "dense"
    assert out["mean_reward"] == np.mean(returns) and out["std_reward"] == np.std(returns)


def test_final_success_rate_with_fewer_and_more_than_ten_rows():
    few = [0.1, 0.2, 0.6]
    assert RC.comparison_from_log(make_log([0.0] * 3, few), "dense")["final_success_rate"] == np.mean(few)
    many = [0.0] * 5 + [0.1 * k for k in range(10)]
    assert RC.comparison_from_log(make_log([0.0] * 15, many), "dense")["final_success_rate"] == np.mean(many[-10:])


def test_rows_without_finished_episodes_are_excluded_from_mean_reward():
    returns = [NAN, 1.0, NAN, 3.0]
    out = RC.comparison_from_log(make_log(returns, [NAN, 0.5, NAN, 1.0]), "sparse")
    assert out["mean_reward"] == 2.0 and out["std_reward"] == 1.0
    assert math.isnan(out["episode_rewards"][0]) and out["episode_rewards"][1] == 1.0
    none = RC.comparison_from_log(make_log([NAN, NAN], [NAN, NAN]), "sparse")
    assert math.isnan(none["mean_reward"]) and math.isnan(none["std_reward"])


def arm(reward_type, step, success_step=None, rows=3):
    log = make_log([0.25] * rows, [0.5] * rows)
    out = RC.comparison_from_log(log, reward_type)
    out["convergence_step"], out["success_convergence_step"] = step, success_step
    return out


def test_report_has_the_improvement_line_only_when_both_arms_converged():
    both = "\n".join(RC.report_lines(arm("sparse", 40), arm("dense", 10)))
    assert "Results Comparison" in both and "Sparse Reward:" in both and "Dense Reward:" in both
    assert "  Mean reward: 0.250 ± 0.000" in both and "  Final success rate: 0.500" in both
    assert "  Convergence step: 40" in both and "  Convergence step: 10" in both
    assert "Convergence improvement: 75.0% faster with dense rewards" in both  # (40 - 10) / 40
    # the reference's ratio divides by the sparse step: a sparse arm converged at step 0 has none
    first = "\n".join(RC.report_lines(arm("sparse", 0), arm("dense", 0)))
    assert "Convergence improvement: n/a" in first and "nan" not in first
    for s, d in ((None, 10), (40, None), (None, None)):
        text = "\n".join(RC.report_lines(arm("sparse", s), arm("dense", d)))
        assert "Convergence improvement" not in text and f"  Convergence step: {s}" in text


def test_json_keys_and_round_trip():
    sparse, dense = arm("sparse", None, 2), arm("dense", 1, 0)
    sparse["episode_rewards"][0] = NAN  # an iteration without a finished episode: null in the file
    res = RC.results_json(sparse, dense)
    assert list(res) == ["sparse", "dense"]
    for name in ("sparse", "dense"):
        assert set(res[name]) == set(RC.REFERENCE_JSON_KEYS + RC.ADDED_JSON_KEYS)
        assert res[name]["reward_type"] == name and res[name]["iterations"] == 3
    assert res["sparse"]["episode_rewards"] == [None, 0.25, 0.25] and res["sparse"]["convergence_step"] is None
    assert res["dense"]["convergence_step"] == 1 and res["sparse"]["success_convergence_step"] == 2
    assert json.loads(json.dumps(res, allow_nan=False)) == res
    # a validated run adds its held-out curve
    dense["validation_iterations"], dense["validation_success_rates"] = [1, 3], [0.25, NAN]
    sparse["validation_iterations"], sparse["validation_success_rates"] = [1, 3], [0.0, 0.5]
    res = RC.results_json(sparse, dense)
    assert set(res["dense"]) == set(RC.REFERENCE_JSON_KEYS + RC.ADDED_JSON_KEYS + RC.VALIDATION_JSON_KEYS)
    assert res["dense"]["validation_success_rates"] == [0.25, None] and res["sparse"]["validation_iterations"] == [1, 3]


def test_run_training_comparison_rejects_an_unknown_reward():
    with pytest.raises(ValueError, match="reward_type"):
        RC.run_training_comparison("shaped", 1)


def test_argument_parsing():
    a = RC.parse_args(["--iterations", "7"])
    assert (a.iterations, a.envs, a.horizon, a.max_steps, a.out, a.validate_every) == (7, 4096, 200, 200, "logs", 0)
    a = RC.parse_args(["--iterations", "3", "--envs", "128", "--horizon", "16", "--max-steps", "13", "--out", "d",
                       "--validate-every", "2"])
    assert (a.iterations, a.envs, a.horizon, a.max_steps, a.out, a.validate_every) == (3, 128, 16, 13, "d", 2)
    assert a.curriculum is None and RC.parse_args(["--iterations", "1", "--curriculum", "hard"]).curriculum == "hard"
    for bad in (["--envs", "8"], ["--iterations", "-1"], ["--iterations", "1", "--envs", "0"],
                ["--iterations", "1", "--curriculum", "steep"]):
        with pytest.raises(SystemExit):
            RC.parse_args(bad)
    need = ["--iterations", "1", "--out", "d"]
    assert train.parse_args(need).reward_type == "dense"
    assert train.parse_args(need + ["--reward-type", "sparse"]).reward_type == "sparse"
    assert train.parse_args(need + ["--config-name", "default", "--reward-type", "sparse"]).config_name == "default"
    for bad in (["--reward-type", "shaped"], ["--config", "f.json", "--reward-type", "sparse"]):
        with pytest.raises(SystemExit):
            train.parse_args(need + bad)
