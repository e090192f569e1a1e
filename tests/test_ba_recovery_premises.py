"""The premises of tests/test_gpu_ba_recovery.py, on the CPU oracle alone: every scene of tests/ba_recovery_cases.py rejects the recorded
iterations, two of them in a row with an accepted step after them, and no accept/reject decision of the oracle sits near the threshold --
conditions on the INPUTS of the GPU tests, met by the reference before anything is asked of the code under test."""
import re

import pytest

import ba_recovery_cases as rc

BA_SCENES = [n for n in rc.SCENES if rc.solver(n) == "ba"]


@pytest.mark.parametrize("name", sorted(rc.SCENES))
def test_oracle_rejects_the_recorded_iterations(oracle_lib, name):
    o = rc.oracle_solve(oracle_lib, name)
    iters = rc.config(name)["bundle_max_iterations"]
    rej = rc.rejected(o["cost_history"])
    assert o["iterations"] == iters and len(o["cost_history"]) == iters + 1
    assert rej == rc.recorded(name)
    assert o["successful_steps"] == iters - len(rej)  # no invalid step, no early stop: every iteration is a step taken or a step rejected
    run = rc.first_run_of_rejections(rej)
    assert run is not None  # two rejections in a row: the second one starts from a point that was linearised on the way back
    assert run[1] + 1 <= iters and run[1] + 1 not in rej  # an accepted step behind the run
    if name == "gen_brown":  # ... and two behind its last rejection
        assert rej[-1] + 2 <= iters


@pytest.mark.parametrize("name", sorted(BA_SCENES))
def test_no_oracle_decision_near_the_acceptance_threshold(oracle_lib, capfd, name):
    """rho = cost change / model change of every iteration, from the oracle's verbose lines: at least 5e-3 from the threshold 1e-3, and on
    the side the cost history shows.  oracle.bundle_general has no verbose output (bundle_general_oracle.cc prints nothing): the two generic
    scenes stay on the pattern check above."""
    capfd.readouterr()
    o = rc.oracle_solve(oracle_lib, name, verbose=True)
    err = capfd.readouterr().err
    rows = re.findall(r"\[ba_oracle\] it (\d+) cost \S+ -> \S+ rho (\S+) radius", err)
    iters = rc.config(name)["bundle_max_iterations"]
    assert [int(r[0]) for r in rows] == list(range(1, iters + 1)), err
    rej = rc.rejected(o["cost_history"])
    assert rej == rc.recorded(name)
    for it, rho in ((int(a), float(b)) for a, b in rows):
        assert abs(rho - rc.RHO_ACCEPT) >= rc.RHO_MARGIN, (it, rho)
        assert (rho <= rc.RHO_ACCEPT) == (it in rej), (it, rho)
