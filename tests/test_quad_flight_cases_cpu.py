"""The conditions tests/quad_flight_cases.py promises about its inputs, held
with the float64 restatement, and the proof that its checker can see a fault.
Runs without a GPU.

  * the float32 free run of every case (no decision forced), put in the
    kernel's place, is accepted for every controller and environment;
  * the float64 free run of the mixed cases decides in every way the rule knows
    (`test_mixed_cases_cover_the_rule`);
  * the float32 restatement under each of ten wrong rules, put in the kernel's
    place, is rejected by at least 10 x the bar it trips (a bitwise or counting
    condition has no bar: its margin is printed as inf)."""
import numpy as np
import pytest
import torch

import quad_flight_cases as Q

F64, F32 = torch.float64, torch.float32
WAVE = 32
WORKGROUP = {"mlp": 256, "lstm": 128, "mlp_learnt": 256, "lstm_learnt": 128}


@pytest.mark.parametrize("name", list(Q.CASES))
def test_float32_free_run_is_accepted(name):
    case = Q.CASES[name]
    for kind in Q.KINDS:
        Q.check(case, kind, Q.as_log(Q.fly(case, kind, F32)))


def test_oracle_closed_loop_runs_in_float64_and_agrees_with_the_restatement():
    """tp.quad_closed_loop (the batched oracle of the older tests) follows its
    input's dtype, and logs what the restatement logs: same rule, written
    twice (the oracle lifts z by 3 m itself)."""
    from oracle import torch_port as tp
    case = Q.CASES[Q.FLAGSHIP]
    for dtype in (F64, F32):
        lowered = case.traj.to(dtype).clone()
        lowered[:, :, 2] -= 3
        ref = tp.quad_closed_loop(Q.controller("mlp", dtype), Q.environment("mlp", dtype),
                                  lowered, Q.DT, Q.H, case.max_steps, case.thresh_div,
                                  case.thresh_stable, case.test_time)
        assert ref["drone"].dtype == ref["div"].dtype == ref["actions"].dtype == dtype
        if dtype == F64:        # (float32: z - 3 + 3 rounds)
            own = Q.free_run(case, "mlp", F64)
            assert torch.equal(ref["steps"], own["steps"])
            for k in ("drone", "div", "actions"):
                assert float((ref[k] - own[k]).abs().max()) < 1e-9, k


# ------------------------------------------------------------------ coverage
def _kinds_of_failure(case, run):
    logged = ~np.isnan(run["div"].numpy())
    td, ts = np.float32(case.thresh_div), np.float32(case.thresh_stable)
    by_div = logged & (run["own_div"].numpy() > td)
    with np.errstate(invalid="ignore"):
        by_att = logged & ((run["roll"].numpy() >= ts) | (run["pitch"].numpy() >= ts))
    return logged, by_div, by_att


@pytest.mark.parametrize("name", Q.MIXED)
def test_mixed_cases_cover_the_rule(name):
    """On the float64 free run.  What a case's geometry cannot hold is left out
    by a rule stated here, not by looking at the run:
      * under test_time a flight starts level and ends at its first failure, so no
        reset ever restores an attitude: attitude-only failures and failures by
        both are asked of the flights without test_time (the `attitude` regime
        flies attitude failures under test_time); they need T >= 4, and a failure
        by both needs L >= 12: the tilted reset row and a jump on the row after it;
      * a reset on the clamped row is observable for L - 11 <= k <= T - 2;
      * with L = 11 every deliberate jump sits on row 1 and the doomed wave fails
        as one at step 0: no mixed step is asked of it."""
    case = Q.CASES[name]
    B, L, _ = case.traj.shape
    T = Q.case_T(case)
    for kind in Q.KINDS:
        run = Q.free_run(case, kind, F64)
        logged, by_div, by_att = _kinds_of_failure(case, run)
        failed = by_div | by_att
        steps = run["steps"].numpy()
        report = dict(case=name, kind=kind, div_only=int((by_div & ~by_att).sum()),
                      attitude_only=int((by_att & ~by_div).sum()),
                      both=int((by_div & by_att).sum()))
        # every full wave: a step with failing and non-failing live flights
        for w in range(B // WAVE):
            if w == Q.DOOMED_WAVE and L == 11:
                continue
            sl = slice(w * WAVE, (w + 1) * WAVE)
            mixed = (failed[sl].any(0) & (logged[sl] & ~failed[sl]).any(0)).any()
            assert mixed, (report, "wave", w)
        assert report["div_only"] > 0, report
        if not case.test_time and T >= 4:
            assert report["attitude_only"] > 0, report
            assert report["both"] > 0 or L == 11, report
        if not case.test_time and T >= L - 9:
            clamped = failed[:, L - 11:T - 1]
            report["clamped_resets"] = int(clamped.sum())
            assert clamped.any(), report
        if case.test_time and T >= 6:
            doomed = slice(Q.DOOMED_WAVE * WAVE, (Q.DOOMED_WAVE + 1) * WAVE)
            assert doomed.stop <= WORKGROUP[kind]        # same workgroup as wave 0
            others = np.r_[steps[:doomed.start], steps[doomed.stop:WORKGROUP[kind]]]
            report["doomed_ends"], report["others_end"] = int(steps[doomed].max()), int(others.max())
            assert steps[doomed].max() <= 4 < others.max(), report
            if kind.startswith("mlp"):     # the recorded LSTM tracks no flight for T steps
                assert others.max() == T, report
        # the inputs keep the decisions away from the thresholds
        stats = Q.check(case, kind, Q.as_log(Q.free_run(case, kind, F32)))
        report.update(decisions=stats["decisions"], in_band=stats["in_band"])
        assert stats["in_band"] <= 0.01 * max(stats["decisions"], 100), report
        print("coverage:", report)


def test_attitude_regime_flies_attitude_failures_under_test_time():
    case = Q.CASES["B300-L40-steps41-attitude-tt1"]
    for kind in Q.KINDS:
        _, by_div, by_att = _kinds_of_failure(case, Q.free_run(case, kind, F64))
        assert by_att.sum() > 100 and not by_div.any(), kind


# --------------------------------------------------------------- wrong rules
TT0, TT1 = Q.FLAGSHIP, "B300-L40-steps41-mixed-tt1"
WRONG = {       # rule -> where it is looked for
    "reset_row_not_clamped": [(TT0, "mlp")],
    "window_advances_off_by_one": [(TT0, "mlp"), (TT1, "mlp")],
    "reset_keeps_body_rates": [(TT0, "mlp")],
    "reset_keeps_attitude": [(TT0, "mlp")],
    "divergence_against_next_row": [(TT0, "mlp"), (TT1, "mlp_learnt")],
    "stability_looks_at_roll_only": [(TT0, "mlp"), (TT0, "lstm")],
    "T_is_min_max_steps_L": [(TT0, "mlp"), (TT1, "mlp")],
    "ended_flight_goes_on_logging": [(TT1, "mlp"), (TT1, "lstm")],
    "lstm_hidden_reset_on_failure": [(TT0, "lstm"), (TT0, "lstm_learnt")],
    "flight_31_flies_flight_30s_window": [(TT0, "mlp"), (TT1, "lstm")],
}


def test_every_wrong_rule_is_listed():
    assert set(WRONG) == set(Q.WRONG_RULES)


@pytest.mark.parametrize("rule", Q.WRONG_RULES)
def test_wrong_rule_is_rejected(rule):
    caught = []
    for name, kind in WRONG[rule]:
        case = Q.CASES[name]
        try:
            Q.check(case, kind, Q.as_log(Q.fly(case, kind, F32, wrong=rule)))
        except Q.Rejected as e:
            caught.append((name, kind, e.what, e.margin))
    assert caught, rule
    name, kind, what, margin = max(caught, key=lambda c: c[3])
    print(f"wrong rule {rule}: rejected on {name}/{kind} by '{what}', {margin:.3g} x its bar")
    assert margin >= 10.0, (rule, caught)
