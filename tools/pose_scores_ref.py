"""CPU reference of mi355ndt_batch_score_poses and of the start-pose search built on it (lv_slam_amd/loop_closure.py: pose_lattice,
pick_starts, verify_candidates_search), through the oracle alone.

  the score of (grid, source, T)   one computeDerivatives sweep (ndt_omp_impl2.hpp:196-305) of the oracle with the source moved by the f32
                                   matrix T: oracle_py.derivatives(grid, source, T, Rj).  The score and the hit count do not depend on Rj
                                   (it enters the gradient and the Hessian alone); the identity is passed.
  the lattice                      entry 0 the guess itself; then for every (ddx, ddy, psi) of dx x dy x dyaw in that order, (0, 0, 0) left
                                   out, [Rz(psi) R | t + (ddx, ddy, 0)] in f64, cast once to f32, last row 0 0 0 1
  the pick                         the highest score; a tie goes to the lowest lattice index (the guess wins ties, and wins when nothing hits)

None of this is in the reference: its loop check aligns from the one guess (loop_detector.hpp:171-172, 250-251).
"""
import numpy as np

from oracle import oracle_py as O

I3 = np.eye(3, dtype=np.float32)


def score(grid: O.Grid, source, T):
    """(score f64, hits int) of one sweep of `source` moved by the 4x4 f32 pose T over `grid`"""
    s, _, _, hits = O.derivatives(grid, np.ascontiguousarray(source, np.float32), np.asarray(T, np.float32), I3)
    return float(s), int(hits)


def scores(grid: O.Grid, source, poses):
    """(scores f64[n], hits int64[n]) of `source` at every pose of [n,4,4]"""
    out = [score(grid, source, T) for T in np.asarray(poses, np.float32).reshape(-1, 4, 4)]
    return np.array([s for s, _ in out], np.float64), np.array([h for _, h in out], np.int64)


def pose_lattice(guess, dx, dy, dyaw):
    """[G,4,4] float32: the guess, then the lattice around it.  Rz(psi) R entry by entry in f64 -- row 0 = c R0 - s R1, row 1 = s R0 + c R1,
    row 2 = R2, every product and every sum rounded where it stands (no library product whose order of operations is its own)."""
    g32 = np.array(guess, np.float32).reshape(4, 4)
    g = g32.astype(np.float64)
    out = [g32]
    for ddx in dx:
        for ddy in dy:
            for psi in dyaw:
                if ddx == 0 and ddy == 0 and psi == 0:
                    continue
                c, s = np.cos(np.float64(psi)), np.sin(np.float64(psi))
                P = np.eye(4)
                for j in range(3):
                    P[0, j] = c * g[0, j] - s * g[1, j]
                    P[1, j] = s * g[0, j] + c * g[1, j]
                    P[2, j] = g[2, j]
                P[0, 3], P[1, 3], P[2, 3] = g[0, 3] + np.float64(ddx), g[1, 3] + np.float64(ddy), g[2, 3]
                P = P.astype(np.float32)
                P[3] = (0, 0, 0, 1)
                out.append(P)
    return np.stack(out)


def pick(row):
    """the lattice index a candidate starts from, given its scores in lattice order"""
    best = 0
    for j, s in enumerate(row):
        if s > row[best]:
            best = j
    return best


def pick_starts(prm: O.Params, target, candidates, guesses, dx, dy, dyaw):
    """(picked lattice index per candidate, the lattices [K,G,4,4], the scores [K,G]) against one target"""
    grid = O.Grid(np.ascontiguousarray(target, np.float32), prm)
    L = np.stack([pose_lattice(g, dx, dy, dyaw) for g in guesses])
    S = np.stack([scores(grid, c, L[k])[0] for k, c in enumerate(candidates)])
    return [pick(r) for r in S], L, S
