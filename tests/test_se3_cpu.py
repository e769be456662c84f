"""CPU: the yardsticks of tests/test_se3_gpu.py checked against each other before anything runs on a device (tests/se3_ref.py).

The oracle's SE(3) functions (oracle/ndt_oracle.c:416-577) are compared, record by record, with
  * the f64 restatement of the same formulas in Python -- same operation order, the C library's sin / cos / tan / atan: equal word for word, so the
    restatement's branch decisions ARE the oracle's (the oracle does not report them);
  * the same formulas at 60 digits (mpmath): the oracle stays within 16 ulp of the largest component, except where (1 - cos theta) / theta^2 cancels:
    there 1 - cos theta carries an absolute error of up to one ulp of 1, i.e. the factor in front of hat(omega) is off by up to min(1/2, 2^-52 / theta^2)
    and the translation by up to that times theta (the bound below allows twice that).  16 ulp: a dozen separately rounded operations of half an ulp each and
    two library functions of up to an ulp each, followed by a 3x3 product."""
import numpy as np

import se3_ref as S

KEY = {1: "M", 2: "p", 3: "p", 4: "p"}
ULP = 2.0 ** -52


def cancellation_allowance(theta):
    return 2.0 * min(0.5, ULP / (theta * theta)) * theta if theta > 0 else 0.0


def test_record_set_covers_every_branch():
    C, R = S.cases(), S.references()
    assert 300 <= len(C) <= 800
    branches = {r["f64"]["branch"] for c, r in zip(C, R) if c["kind"] in (2, 3) and c["cls"] != "nan"}
    assert branches == {0, 1, 2, 3}                                            # trace > 0 and each of the three sub-branches of trace <= 0
    init_branches = {r["f64"]["branch"] for c, r in zip(C, R) if c["kind"] == 3 and c["cls"] != "nan"}
    assert init_branches == {0, 1, 2, 3}
    logs = [r["f64"] for c, r in zip(C, R) if c["kind"] in (2, 3, 4) and c["cls"] != "nan"]
    assert any(r["n_small"] for r in logs if "n_small" in r) and any(r["theta_small"] and r["theta"] < -1.0 for r in logs)   # signed theta: a large negative angle, small-angle V^-1
    assert any(r["f64"]["small"] for c, r in zip(C, R) if c["kind"] == 1 and c["cls"] != "nan")
    comp = [r["f64"] for c, r in zip(C, R) if c["kind"] == 4 and c["cls"] != "nan"]
    assert sum(r["w"] < 0 for r in comp) >= 8                                  # products whose quaternion has w < 0
    ties = [c for c in C if c["kind"] == 2 and c["R"][4] == c["R"][0] and c["R"][0] + c["R"][4] + c["R"][8] <= 0]
    assert ties


def test_f64_restatement_is_the_oracle_word_for_word():
    for c, r in zip(S.cases(), S.references()):
        if c["kind"] == 0:
            continue
        assert np.array_equal(r["f64"][KEY[c["kind"]]], r["ora"], equal_nan=True), (c["kind"], c["cls"], c["rec"])
        if c["kind"] == 3:
            assert np.array_equal(r["f64"]["R"], r["ora_R"], equal_nan=True)


def test_oracle_against_sixty_digits():
    worst = {}
    for c, r in zip(S.cases(), S.references()):
        k = c["kind"]
        if k == 0 or c["cls"] == "nan":
            continue
        err, ulp = S.scaled_err(r["ora"], r["mp"][KEY[k]])
        theta = float(np.linalg.norm(c["p"][3:6])) if k in (1, 4) else 0.0    # only the exponential cancels
        assert err <= 16 * max(ulp, ULP) + cancellation_allowance(theta), (k, c["cls"], err, theta)
        worst[(k, c["cls"])] = max(worst.get((k, c["cls"]), 0.0), err)
        if k == 3:
            assert S.scaled_err(r["ora_R"], r["mp"]["R"])[0] <= 16 * ULP
    # outside the cancellation-limited classes the oracle is a few ulp from the exact value: a yardstick that means something
    for (k, cls), e in worst.items():
        if not (k in (1, 4) and cls in ("cancel", "mid")):
            assert e <= 16 * ULP, (k, cls, e)


def test_nan_records_give_nan_in_the_oracle():
    n = 0
    for c, r in zip(S.cases(), S.references()):
        if c["cls"] == "nan":
            assert np.isnan(r["ora"]).any()
            n += 1
    assert n == 4
