"""The conditions tests/wing_flight_cases.py promises about its inputs, held
with the float64 restatement, and the proof that its checker can see a fault.
Runs without a GPU.

  * the float32 free run of every case (no decision forced), put in the
    kernel's place, is accepted for both environments - with room: decisions
    inside BAND are at most 1 % of those observed, the float32 restatement is
    within BAND / 4 of float64 on every distance and deciding quantity and within
    2.5e-5 per flight in every column group (so that four times its error fits
    under the suite's 1e-4);
  * the float64 free run of the mixed cases decides in every way the rule knows
    (`test_mixed_cases_cover_the_rule`);
  * oracle.torch_port.wing_closed_loop, the earlier statement of the rule,
    agrees with the restatement;
  * the float32 restatement under each of twelve wrong rules, put in the
    kernel's place, is rejected by at least 10 x the bar it trips (a bitwise or
    counting condition has no bar: its margin is printed as inf)."""
import numpy as np
import pytest
import torch

import wing_flight_cases as W

F64, F32 = torch.float64, torch.float32
WORKGROUP = 256
ROOM = 2.5e-5          # x FACTOR = 4: the suite's 1e-4 per flight


@pytest.mark.parametrize("name", W.NAMES)
def test_float32_free_run_is_accepted_with_room(name):
    for kind in W.KINDS:
        case = W.get(name, kind)
        stats = W.check(case, kind, W.as_log(W.free_run(case, kind, F32)))
        room = {g: float("%.3g" % stats[g]["worst_f32"]) for g, _, _ in W.GROUPS}
        report = dict(case=case.name, decisions=stats["decisions"], in_band=stats["in_band"],
                      div_abs=float("%.3g" % stats["div_abs"]),
                      q_abs=float("%.3g" % stats["q_abs_f32"]), **room)
        print("room:", report)
        assert stats["in_band"] <= 0.01 * max(stats["decisions"], 100), report
        assert stats["div_abs"] <= W.BAND / 4 and stats["q_abs_f32"] <= W.BAND / 4, report
        assert max(room.values()) <= ROOM, report


def test_first_pass_of_the_flights_as_drawn():
    """The max_steps cases sit around FIRST_PASS: no flight outside the short
    wave and the constructed ones passes a target before that step, the calm
    ones pass their first target on it."""
    for kind in W.KINDS:
        case = W.get(W.FLAGSHIP, kind)
        passed = W.free_run(case, kind, F64)["div_pass"].numpy() >= 0
        b = np.arange(passed.shape[0])
        drawn = (b // W.WAVE != W.SHORT_WAVE) & ~np.isin(b % 16, list(W.CONSTRUCTED))
        first = np.where(passed.any(1), passed.argmax(1), 10 ** 6)
        assert first[drawn].min() == W.FIRST_PASS, (kind, first[drawn].min())
        assert (first[drawn & (b % 16 == 0)] == W.FIRST_PASS).all(), kind


def test_oracle_closed_loop_agrees_with_the_restatement():
    """tp.wing_closed_loop (the batched oracle of the older tests: float32 state
    path, float64 geometry) logs what the float64 restatement logs - steps and
    events equal, numbers to 1e-4 of each column group's scale: same rule,
    written twice."""
    from oracle import torch_port as tp
    d = W.data()
    case = W.get(W.FLAGSHIP, "wing")
    ref = tp.wing_closed_loop(W.controller(F32), W.environment("wing", F32), case.targets, d["dt"],
                              d["mean"], d["std"], d["data_dt"], d["data_horizon"],
                              case.max_steps, case.thresh_div, case.thresh_stable, case.test_time,
                              state0=case.state0)
    own = W.free_run(case, "wing", F64)
    assert torch.equal(ref["steps"], own["steps"])
    logged = ~torch.isnan(own["div_linear"])
    for k in ("div_pass", "div_fail"):
        assert torch.equal((ref[k] >= 0) & logged, own[k] >= 0), k
        event = own[k] >= 0
        assert float((ref[k] - own[k])[event].abs().max()) < W.BAND, k
    assert float((ref["div_linear"] - own["div_linear"])[logged].abs().max()) < W.BAND
    for group, name, cols in W.GROUPS:
        mine = own[name][:, :, cols]
        theirs = ref["traj" if name == "drone" else "seen"][:, :, cols].double()
        err = torch.where(logged[:, :, None], (theirs - mine).abs(), torch.zeros_like(mine))
        scale = torch.where(logged[:, :, None], mine.abs(), torch.zeros_like(mine)).amax((1, 2))
        assert float((err.amax((1, 2)) / scale).max()) < 1e-4, group


# ------------------------------------------------------------------ coverage
def _events(case, run):
    T = case.max_steps
    logged = ~np.isnan(run["div_linear"].numpy())
    passed, failed = run["div_pass"].numpy() >= 0, run["div_fail"].numpy() >= 0
    with np.errstate(invalid="ignore"):
        by_div = failed & (run["q_div"].numpy() > 0)
        by_att = failed & ((run["q_roll"].numpy() >= 0) | (run["q_pitch"].numpy() >= 0))
    return logged, passed, failed, by_div, by_att


@pytest.mark.parametrize("name", W.MIXED)
def test_mixed_cases_cover_the_rule(name):
    """On the float64 free run.  What a case's geometry cannot hold is left out
    by a rule stated here, not by looking at the run:
      * a flight that starts on its line with at most 3 m/s across it is 0.9 m
        off after six steps at the earliest, and a second failure needs as many
        again: failures by divergence, failures after a switch and second
        resets are asked of the cases that fly T_FULL steps; so are the passes
        that end a flight (the short wave's at step 5) and the constructed
        flights' pass-and-failure (at the first failing step, by divergence);
      * a switch needs a second target, and T > FIRST_PASS; with one target a
        flight ends at its first pass, four to six steps in: no second reset;
      * with the zero reset (state0 = None) every flight starts level on its
        line at 11.5 m/s: no start state tilts or pushes one sideways, so only
        what the targets decide is asked (switch, ending pass)."""
    B, n_t, T, _, tt, with_state0 = (W.SPECS[name] + (True,))[:6]
    for kind in W.KINDS:
        case = W.get(name, kind)
        run = W.free_run(case, kind, F64)
        logged, passed, failed, by_div, by_att = _events(case, run)
        steps = run["steps"].numpy()
        last = run["last"].numpy()
        report = dict(case=case.name, div_only=int((by_div & ~by_att).sum()),
                      attitude_only=int((by_att & ~by_div).sum()),
                      switches=int((passed & ~last).sum()), ending_passes=int((passed & last).sum()),
                      pass_and_failure=int((passed & failed).sum()))
        full = T == W.T_FULL
        if with_state0:
            # every full wave: a step with failing and non-failing live flights
            for w in range(B // W.WAVE):
                sl = slice(w * W.WAVE, (w + 1) * W.WAVE)
                mixed = (failed[sl].any(0) & (logged[sl] & ~failed[sl]).any(0)).any()
                assert mixed, (report, "wave", w)
            assert report["attitude_only"] > 0, report
            if full:
                assert report["div_only"] > 0, report
        if n_t > 1 and T > W.FIRST_PASS:
            assert report["switches"] > 0, report
        if full:
            assert report["ending_passes"] > 0, report
        if full and n_t > 1 and with_state0:
            assert report["pass_and_failure"] > 0 and (passed & failed & ~last).any(), report
            first_switch = np.where((passed & ~last).any(1), (passed & ~last).argmax(1), T)
            after = failed & (np.arange(T)[None, :] > first_switch[:, None])
            report["failures_after_a_switch"] = int(after.sum())
            assert after[np.arange(B) % 16 == 5].any(), report
        if full and n_t > 1 and with_state0 and not tt:
            report["most_resets"] = int(failed.sum(1).max())
            assert report["most_resets"] >= 2, report
        if full and tt:
            short = slice(W.SHORT_WAVE * W.WAVE, (W.SHORT_WAVE + 1) * W.WAVE)
            others = np.r_[0:short.start, short.stop:min(B, WORKGROUP)]
            went_on = (steps[others] == T) | ((passed & last).any(1)[others]
                                              & (steps[others] > steps[short].max()))
            report["short_wave_ends"] = int(steps[short].max())
            assert steps[short].max() <= 12 and went_on.any(), report
        print("coverage:", report)


def test_attitude_regime_flies_attitude_failures_under_test_time():
    for kind in W.KINDS:
        case = W.get(f"B300-n3-steps{W.T_FULL}-attitude-tt1", kind)
        _, _, _, by_div, by_att = _events(case, W.free_run(case, kind, F64))
        assert by_att.sum() > 100 and not by_div.any(), kind


def test_everybody_regime_fails_at_every_step_by_a_whole_unit():
    for kind in W.KINDS:
        case = W.get("B300-n3-steps12-everybody-tt0", kind)
        run = W.free_run(case, kind, F64)
        logged, passed, failed, _, _ = _events(case, run)
        assert (failed | (passed & run["last"].numpy()))[logged].all(), kind
        assert min(run["q_roll"][logged].min(), run["q_pitch"][logged].min()) >= 1.0, kind


# --------------------------------------------------------------- wrong rules
TT0, TT1 = W.FLAGSHIP, W.FLAGSHIP_TT1
WRONG = {       # rule -> where it is looked for
    "policy_sees_the_reset_state": [(TT0, "wing")],
    "reset_towards_the_new_target": [(TT0, "wing"), (TT0, "wing_learnt")],
    "line_not_moved_on_switch": [(TT0, "wing"), (TT1, "wing_learnt")],
    "miss_distance_from_line_start": [(TT0, "wing"), (TT1, "wing")],
    "failure_tested_after_the_last_target": [(TT0, "wing"), (TT1, "wing_learnt")],
    "stability_looks_at_roll_only": [(TT0, "wing"), (TT1, "wing_learnt")],
    "reset_keeps_body_rates": [(TT0, "wing")],
    "reset_speed_is_the_current_speed": [(TT0, "wing"), (TT0, "wing_learnt")],
    "test_time_logs_thresh_div": [(TT1, "wing"), (TT1, "wing_learnt")],
    "ended_flight_goes_on_logging": [(TT1, "wing"), (TT0, "wing_learnt")],
    "flight_31_flies_flight_30s_targets": [(TT0, "wing"), (TT1, "wing_learnt")],
    "target_index_shared_by_the_wave": [(TT0, "wing"), (TT1, "wing_learnt")],
}


def test_every_wrong_rule_is_listed():
    assert set(WRONG) == set(W.WRONG_RULES)


@pytest.mark.parametrize("rule", W.WRONG_RULES)
def test_wrong_rule_is_rejected(rule):
    caught = []
    for name, kind in WRONG[rule]:
        case = W.get(name, kind)
        try:
            W.check(case, kind, W.as_log(W.fly(case, kind, F32, wrong=rule)))
        except W.Rejected as e:
            caught.append((name, kind, e.what, e.margin))
    assert caught, rule
    name, kind, what, margin = max(caught, key=lambda c: c[3])
    print(f"wrong rule {rule}: rejected on {name}/{kind} by '{what}', {margin:.3g} x its bar")
    assert margin >= 10.0, (rule, caught)
