"""CPU: the host-side pieces of the start-pose search (lv_slam_amd/loop_closure.py: pose_lattice, pick_starts) against their restatement
(tools/pose_scores_ref.py) and against matrices written out by hand.  The kernels and mi355ndt_batch_score_poses: tests/test_pose_scores_gpu.py."""
import numpy as np
import pytest

from lv_slam_amd import loop_closure as LC
from lv_slam_amd import ndt
from tools import pose_scores_ref as R


def a_guess(seed=3):
    """a rigid f32 pose with every entry busy: yaw, a little roll and pitch, a translation"""
    rng = np.random.default_rng(seed)
    a, b, c = 0.7, 0.05, -0.03
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
    G = np.eye(4)
    G[:3, :3] = Rz @ Ry @ Rx
    G[:3, 3] = rng.normal(0, 3, 3)
    G[2, 3] = 0.0
    return G.astype(np.float32)


OFFSETS = [((-1.0, 0.0, 1.0), (-1.0, 0.0, 1.0), (-0.1, 0.0, 0.1)),       # (0, 0, 0) among the combinations
           ((0.5, 1.0), (0.0,), (0.0, 0.2)),                              # ... and not
           ((0.0,), (0.0,), (0.0,)),                                      # the lattice of one pose
           ((), (1.0,), (0.0,))]                                          # an empty list: the guess alone


@pytest.mark.parametrize("dx,dy,dyaw", OFFSETS)
def test_entry_zero_is_the_guess_and_the_count(dx, dy, dyaw):
    G = a_guess()
    L = LC.pose_lattice(G, dx=dx, dy=dy, dyaw=dyaw)
    assert L.dtype == np.float32 and L.shape[1:] == (4, 4)
    assert L[0].tobytes() == G.tobytes()                                   # bit for bit, whatever the lists hold
    combos = len(dx) * len(dy) * len(dyaw)
    has_zero = 0.0 in dx and 0.0 in dy and 0.0 in dyaw
    assert len(L) == 1 + combos - (1 if has_zero else 0)
    # the (0, 0, 0) combination is not repeated: no later entry is the guess again
    assert not any(P.tobytes() == G.tobytes() for P in L[1:])


@pytest.mark.parametrize("dx,dy,dyaw", OFFSETS)
def test_last_rows_are_exact_and_the_restatement_agrees(dx, dy, dyaw):
    G = a_guess(5)
    L = LC.pose_lattice(G, dx=dx, dy=dy, dyaw=dyaw)
    assert all(P[3].tobytes() == np.float32([0, 0, 0, 1]).tobytes() for P in L)
    assert L.tobytes() == R.pose_lattice(G, dx, dy, dyaw).tobytes()


def test_default_lattice_is_five_by_five_by_three():
    L = LC.pose_lattice(np.eye(4, dtype=np.float32))
    assert len(L) == 5 * 5 * 3 and L[0].tobytes() == np.eye(4, dtype=np.float32).tobytes()


def test_quarter_turn_on_a_known_guess():
    """guess: a quarter turn about z already, t = (1, 2, 3).  One more quarter turn and (+2, -1): R = Rz(pi), t = (3, 1, 3).  cos(pi/2) in f64 is
    6.1e-17, so the f64 products differ from the exact matrix by less than one f32 rounding of their entries."""
    G = np.array([[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]], np.float32)
    L = LC.pose_lattice(G, dx=(2.0,), dy=(-1.0,), dyaw=(np.pi / 2,))
    assert len(L) == 2
    c = np.float32(np.cos(np.pi / 2))                                      # 6.123234e-17: Rz(pi/2)'s diagonal as f64 has it, cast
    want = np.array([[-1, -c, 0, 3], [c, -1, 0, 1], [0, 0, 1, 3], [0, 0, 0, 1]], np.float32)
    assert L[1].tobytes() == want.tobytes(), (L[1], want)
    # the translation is offset in the target's frame, not rotated
    assert L[1][0, 3] == 3 and L[1][1, 3] == 1 and L[1][2, 3] == 3


def test_the_pick_rule():
    S = np.array([[0.0, 0.0, 0.0, 0.0],           # nothing hits: the guess
                  [1.0, 3.0, 3.0, 2.0],           # a tie: the lowest index
                  [5.0, 5.0, 1.0, 5.0],           # a tie with the guess: the guess
                  [1.0, 2.0, 3.0, 4.0]])
    assert LC.pick_starts(S) == [0, 1, 0, 3]
    assert [R.pick(list(r)) for r in S] == [0, 1, 0, 3]
    assert LC.pick_starts(np.zeros((2, 1))) == [0, 0]


def test_the_symbol_and_the_surface_exist():
    assert "mi355ndt_batch_score_poses" in ndt.SYMBOLS
    assert callable(getattr(ndt.Engine, "batch_score_poses")) and callable(LC.verify_candidates_search)
    assert ndt.SCORE_POSES_MAX_ITEMS == 65536
