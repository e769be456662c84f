"""GPU (-m gpu): the SE(3) pose math of the Newton control on the device (lv_slam_amd/csrc/ndt_math.hpp, init_pair_state and newton_rebase of
ndt_newton.hpp; Sophus a621ff2 / Eigen 3.3 restated, ndt_omp_impl2.hpp:102-129, 163-166) at the angles no align in the suite reaches: around the 1e-10
small-angle threshold, beyond 120 degrees (the trace <= 0 branch of the matrix -> quaternion conversion with its three sub-branches), w -> 0 and w < 0
(where the SIGNED `theta < 1e-10` test of SE3::log takes the small-angle V^-1 for a large negative angle: the reference's Sophus, so a contract), half
turns, f32-rounded guesses, translations from 0 to 1e5 m.  tests/hip/se3_check (built by build()) evaluates the records of tests/se3_ref.py on the device.

Bars:
  * what is only add / multiply / divide / square root (the quaternion and matrix helpers): equal word for word to the f64 restatement in the same order;
  * newton_rebase on a full wave (two exponentials side by side on lanes 0 and 1, exchanged by shuffles) == the same on one lane: word for word;
  * exp / log / init_pair_state call sin, cos, tan, atan, and the device's are not the C library's.  Device, oracle and the same formulas at 60 digits
    (mpmath, same branch rules) are compared per input class: the device's largest error against the 60-digit value is at most FOUR times the oracle's
    plus 4 ulp of the result's largest component (errors scaled by max(1, largest |component|)).  Four = two library functions in a chain, each allowed twice
    the C library's error.  The cancellation-limited classes ("cancel": theta from 1e-10 to 1e-5, and "mid": theta = 1e-3, where (1 - cos theta) / theta^2 still loses
    digits on any libm) are classes of their own, with the oracle's measured error as the yardstick.  The composition log(exp(dp) exp(p)) chains three (exp, exp, log): factor six.
  * every branch decision equals the oracle's (= the f64 restatement's, which tests/test_se3_cpu.py holds equal to the oracle word for word).  The
    small-angle decisions come out of the library's own so3_exp / so3_log; where the quaternion's vector part is below 1e-10 theta is add / multiply /
    divide only, so the decision AND theta are held word for word, the records at 9.9e-11, 1e-10 and 1.1e-10 included.  Only where theta went through the
    device's atan and lies within a factor 2 of the threshold is the decision left open (no record does today).  The reported q_from_matrix branch is the
    check program's own restatement of the comparisons on the same operands: what guards the library's branch is its result, word for word, in kind 0.
    Likewise the reported small-angle flags compare the library's theta with the library's NDT_SMALL_EPS in the check program.  se3_exp's own use of the
    decision is visible in its result at the threshold (theta / 2 of the translation) and is asserted there; se3_log's is not -- the two formulas for V^-1
    differ by theta^2 / 12 = 1e-21 of the translation at 1e-10, below any f64 comparison -- so for the logarithm theta itself, word for word, is what can be held.
Measured figures: docs/experiments.md 10k."""
import subprocess
import numpy as np
import pytest

import se3_ref as S

pytestmark = pytest.mark.gpu
F32_HALF_ULP = 2.0 ** -25            # |x| <= 1 rounded to f32


@pytest.fixture(scope="module")
def dev(tmp_path_factory):
    import __graft_entry__ as entry
    exe = entry.build_se3_check()
    d = tmp_path_factory.mktemp("se3")
    S.write_records(d / "in.f64")
    subprocess.check_call([exe, str(d / "in.f64"), str(d / "out.f64")], timeout=120)       # NaN records included: the program ends
    out = np.fromfile(d / "out.f64", np.float64).reshape(-1, S.REC_OUT)
    assert len(out) == len(S.cases())
    return out


def near_threshold(theta):
    """within a factor 2 of the small-angle threshold: there a theta that went through the device's atan may decide otherwise (both formulas agree to 1e-20)"""
    return 0.5e-10 < abs(theta) < 2e-10


def rows(dev, kind, with_nan=False):
    return [(c, r, o) for c, r, o in zip(S.cases(), S.references(), dev) if c["kind"] == kind and (with_nan or c["cls"] != "nan")]


def class_bar(items, factor, label):
    """items: (cls, device value, oracle value, 60-digit value).  Per class: max device error <= factor * max oracle error + 4 ulp."""
    E = {}
    for cls, d, o, m in items:
        ed, ulp = S.scaled_err(d, m)
        eo, _ = S.scaled_err(o, m)
        e = E.setdefault(cls, [0.0, 0.0, 0.0, 0, 0])
        e[0], e[1], e[2], e[3] = max(e[0], ed), max(e[1], eo), max(e[2], ulp), e[3] + 1
        e[4] += not np.array_equal(d, o)
    bad = []
    for cls in sorted(E):
        ed, eo, ulp, n, ndiff = E[cls]
        print(f"se3 {label:8s} {cls:7s} n={n:3d} device {ed:.3e} oracle {eo:.3e} bar {factor * eo + 4 * ulp:.3e}  (words differ from the oracle's in {ndiff} records)")
        if not ed <= factor * eo + 4 * ulp:
            bad.append((cls, ed, eo))
    assert not bad, (label, bad)


def test_quaternion_and_matrix_helpers_word_for_word(dev):
    """q_from_matrix, q_normalized, q_to_matrix, q_mul, q_rotate, se3_mul, mat3_inverse: IEEE add / multiply / divide / sqrt only"""
    R = rows(dev, 0)
    assert len(R) > 150
    names = [("q_from_matrix", 0, 4), ("branch", 4, 5), ("q_normalized", 5, 9), ("q_to_matrix", 9, 18), ("q_normalized(q2)", 18, 22), ("q_mul", 22, 26),
             ("q_rotate", 26, 29), ("se3_mul", 29, 36), ("mat3_inverse", 36, 45)]
    for c, r, o in R:
        for name, a, b in names:
            assert np.array_equal(o[a:b], r["f64"][a:b]), (name, c["cls"], c["m"], o[a:b], r["f64"][a:b])
    assert {int(o[4]) for _, _, o in R} == {0, 1, 2, 3}


def test_rebase_on_a_wave_equals_one_lane(dev):
    """newton_rebase: lanes 0 and 1 exponentiate dp and p side by side; a mix-up of the two is invisible while both rotations are tiny"""
    R = rows(dev, 4, with_nan=True)
    for c, r, o in R:
        assert np.array_equal(o[0:6], o[22:28], equal_nan=True), (c["cls"], c["p"], c["dir"], c["a_t"], o[0:6], o[22:28])
    assert sum(o[28] < 0 for _, _, o in R) >= 8                                          # products with w < 0 are among them
    # inc_cm = float(exp(dp).matrix()), column-major
    for c, r, o in rows(dev, 4):
        inc = o[6:22].reshape(4, 4).T
        want = r["mp"]["inc"]
        scale = max(1.0, np.abs(want).max())
        assert np.abs(np.concatenate([inc[:3, :3].ravel(), inc[:3, 3]]) - want).max() <= (2 * F32_HALF_ULP + 1e-14) * scale
        assert np.array_equal(inc[3], [0, 0, 0, 1])


def test_exp_against_oracle_and_sixty_digits(dev):
    R = rows(dev, 1)
    class_bar([(c["cls"], np.concatenate([o[8:17], o[4:7]]), r["ora"], r["mp"]["M"]) for c, r, o in R], 4, "exp")
    for c, r, o in R:
        assert bool(o[7]) == r["f64"]["small"], (c["p"], o[7])                           # theta is add / multiply / sqrt only: the same decision
        # pose_to_f32: T = [R | t] row-major 3x4 and Rj = R, each the f32 rounding of the f64 value the device computed itself
        Rd, td = o[8:17].reshape(3, 3), o[4:7]
        T, Rj = o[17:29].reshape(3, 4), o[29:38].reshape(3, 3)
        assert np.array_equal(T[:, :3], Rd.astype(np.float32).astype(np.float64)) and np.array_equal(T[:, 3], td.astype(np.float32).astype(np.float64))
        assert np.array_equal(Rj, Rd.astype(np.float32).astype(np.float64)), (c["p"], Rj, Rd)
    assert any(np.abs(o[29:38].reshape(3, 3) - o[29:38].reshape(3, 3).T).max() > 0.5 for _, _, o in R)   # (a transposed Rj would show)
    # se3_exp's own decision at the threshold shows in its result: the small branch takes V = R = I + hat(omega) + ..., the other one
    # V = I + a hat(omega) + ... with a = (1 - cos theta) / theta^2 = 0 there on any libm (cos theta rounds to 1), so the translation moves by theta / 2 of
    # |upsilon| (5e-11, far inside the "cancel" class's bar).  Same branch, same operations, library functions an ulp apart at most: 16 ulp.
    at = [(c, r, o) for c, r, o in R if near_threshold(float(np.linalg.norm(c["p"][3:6]))) and np.abs(c["p"][:3]).max() > 0]
    for c, r, o in at:
        err, ulp = S.scaled_err(np.concatenate([o[8:17], o[4:7]]), r["ora"])
        assert err <= 16 * max(ulp, 2.0 ** -52), (c["p"], err)
    small = [r["f64"]["small"] for _, r, _ in at]
    assert len(at) >= 12 and any(small) and not all(small)


def test_log_against_oracle_and_sixty_digits(dev):
    R = rows(dev, 2)
    class_bar([(c["cls"], o[0:6], r["ora"], r["mp"]["p"]) for c, r, o in R], 4, "log")
    for c, r, o in R:
        f = r["f64"]
        assert int(o[6]) == f["branch"], (c["R"], o[6], f["branch"])
        assert bool(o[7]) == f["n_small"], (c["R"], o[7])
        if f["n_small"]:                                                                  # theta = f n without atan: the same words, the same decision
            assert np.array_equal(o[9], f["theta"], equal_nan=True) and bool(o[8]) == f["theta_small"], (c["R"], o[9], f["theta"])
        elif not near_threshold(f["theta"]):
            assert bool(o[8]) == f["theta_small"], (c["R"], o[9], f["theta"])
    assert any(bool(o[8]) and o[9] < -1.0 for _, _, o in R)                              # large negative angle, small-angle V^-1: reached on the device
    at = [bool(o[8]) for c, r, o in R if r["f64"]["n_small"] and near_threshold(r["f64"]["theta"])]
    assert len(at) >= 18 and any(at) and not all(at)                                     # both outcomes right at the threshold


def test_init_pair_state_against_oracle_and_sixty_digits(dev):
    R = rows(dev, 3)
    class_bar([(c["cls"], o[0:6], r["ora"], r["mp"]["p"]) for c, r, o in R], 4, "init")
    for c, r, o in R:
        G = c["G"].astype(np.float64)
        assert np.array_equal(o[6:18].reshape(3, 4), G[:3, :4])                           # the first sweep moves the cloud by the guess itself
        f = r["f64"]
        assert int(o[27]) == f["branch"]
        if f["n_small"]:
            assert np.array_equal(o[29], f["theta"], equal_nan=True) and bool(o[28]) == f["theta_small"], (c["G"], o[29], f["theta"])
        elif not near_threshold(f["theta"]):
            assert bool(o[28]) == f["theta_small"]
        # Rj = float(rotation of exp(p)): the 60-digit rotation, rounded once to f32, with the f64 error of p and exp on top
        assert np.abs(o[18:27] - r["mp"]["R"]).max() <= F32_HALF_ULP + 1e-14, (c["G"], o[18:27], r["mp"]["R"])
    assert {int(o[27]) for _, _, o in R} == {0, 1, 2, 3}
    at = [bool(o[28]) for c, r, o in R if r["f64"]["n_small"] and near_threshold(r["f64"]["theta"])]
    assert len(at) >= 18 and any(at) and not all(at)


def test_compose_against_oracle_and_sixty_digits(dev):
    """p_new = log(exp(dp) exp(p)) (ndt_omp_impl2.hpp:166) on one lane, against the oracle's se3_compose_log"""
    R = rows(dev, 4)
    class_bar([(c["cls"], o[22:28], r["ora"], r["mp"]["p"]) for c, r, o in R], 6, "compose")
    for c, r, o in R:
        f = r["f64"]
        if abs(f["w"]) > 1e-12:
            assert (o[28] < 0) == (f["w"] < 0)
        if not near_threshold(f["theta"]) and abs(f["w"]) > 1e-12:                       # (the product's quaternion went through the device's sin / cos / atan)
            assert bool(o[29]) == f["theta_small"], (c["p"], c["dir"], c["a_t"], o[30], f["theta"])


def test_nan_in_nan_out(dev):
    """a NaN tangent, a NaN guess entry: NaN comes out where the oracle gives NaN (and the program ended: the fixture read its file)"""
    n = 0
    for c, r, o in zip(S.cases(), S.references(), dev):
        if c["cls"] != "nan":
            continue
        n += 1
        if c["kind"] == 1:
            got = np.concatenate([o[8:17], o[4:7]])
        elif c["kind"] == 4:
            got = o[22:28]
            assert np.array_equal(np.isnan(o[0:6]), np.isnan(r["ora"]))
        else:
            got = o[0:6]
            assert np.array_equal(np.isnan(o[6:18].reshape(3, 4)), np.isnan(c["G"][:3, :4]))
        assert np.array_equal(np.isnan(got), np.isnan(r["ora"])), (c["kind"], got, r["ora"])
        assert np.isnan(r["ora"]).any()
    assert n == 4
