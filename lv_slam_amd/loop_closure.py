"""Loop-closure verification on the batch surfaces (NDT: verify_candidates; GICP: verify_candidates_gicp).

The reference's loop detector (include/global_graph/loop_detector.hpp) verifies the candidate keyframes of a new keyframe one by one: the
new keyframe is the target, every candidate in turn is the source, aligned from the guess `new.inverse() * candidate` (z zeroed) and
scored with getFitnessScore(fitness_score_max_range); the converged candidate with the lowest score wins if that score is within
fitness_score_thresh.  `matching` (:148-205) walks all candidates; `matching_and_bow` (:211-281) walks the DBoW3 top results in BoW
order and stops early.

Every align of that loop is independent of the others given the target: what one candidate yields does not depend on which candidates
were aligned before it.  So aligning all K candidates in ONE batch (mi355ndt_batch_align), scoring them in one call
(mi355ndt_batch_fitness_scores) and then applying the reference's selection rule to the precomputed (converged, score, final) triples
selects the same loop, with the same relative pose and score, as the reference's sequential loop.  The rules below also report how many
aligns the sequential loop would have run (matching_and_bow stops early; the batch aligns every candidate it was given).
"""
from __future__ import annotations

import numpy as np

from . import ndt

DBL_MAX = 1.7976931348623157e308
BOW_MIN_SCORE = 0.04            # matching_and_bow: a BoW score below this ends the walk (loop_detector.hpp:240)


def loop_guess(new_pose, cand_pose) -> np.ndarray:
    """(new_pose.inverse() * cand_pose).matrix().cast<float>() with guess(2, 3) = 0 (loop_detector.hpp:171-172, 250-251).
    The poses are the keyframes' 4x4 isometries (node estimates, f64); the inverse is the rigid one, [R^T, -R^T t]."""
    N = np.asarray(new_pose, np.float64)
    Cp = np.asarray(cand_pose, np.float64)
    if N.shape != (4, 4) or Cp.shape != (4, 4):
        raise ValueError("poses must be 4x4")
    inv = np.eye(4)
    inv[:3, :3] = N[:3, :3].T
    inv[:3, 3] = -(N[:3, :3].T @ N[:3, 3])
    G = (inv @ Cp).astype(np.float32)
    G[3] = np.float32([0, 0, 0, 1])
    G[2, 3] = 0.0
    return G


def select_matching(converged, scores, finals, thresh: float):
    """LoopDetector::matching's rule (loop_detector.hpp:168-197) over precomputed per-candidate results, in candidate order.
    A candidate is skipped when it has not converged or its score is above the best so far, so a tie goes to the LATER candidate.
    Returns (index or None, relative_pose or None, best_score, aligns the reference would have run); None when best_score > thresh."""
    best, idx, pose = DBL_MAX, None, None
    for i, (c, s) in enumerate(zip(converged, scores)):
        if not c or s > best:
            continue
        best, idx, pose = float(s), i, np.asarray(finals[i])
    if best > thresh:
        return None, None, best, len(scores)
    return idx, pose, best, len(scores)


def select_matching_and_bow(converged, scores, finals, bow, thresh: float):
    """LoopDetector::matching_and_bow's rule (loop_detector.hpp:240-270).  `bow` = the DBoW3 query results in their order, as
    (bow_score, candidate index) pairs.  Before each candidate the walk ends when its BoW score is below 0.04 or the best score so far
    is already within `thresh`; otherwise the candidate counts as aligned, and is skipped when it has not converged or scores above
    the best.  Returns (index or None, relative_pose or None, best_score, aligns the reference would have run)."""
    best, matched, pose, aligns = DBL_MAX, None, None, 0
    for b, cid in bow:
        if b < BOW_MIN_SCORE or best <= thresh:
            break
        # the reference assigns best_matched before it checks the candidate (:246-247); once the best score is within `thresh` the
        # next round ends the walk, so a loop that is returned always names the candidate that gave best_score
        matched = int(cid)
        aligns += 1
        if not converged[cid] or scores[cid] > best:
            continue
        best, pose = float(scores[cid]), np.asarray(finals[cid])
    if best > thresh:
        return None, None, best, aligns
    return matched, pose, best, aligns


def verify_candidates(engine: ndt.Engine, target, candidates, guesses, max_range: float = float("inf"), thresh: float = 0.5, bow=None):
    """Verify loop candidates against one new keyframe on the batch surface: the target in every slot, candidate k as the source of
    slot k, ONE batch_align from `guesses` ([K,4,4], e.g. loop_guess per candidate), ONE batch_fitness_scores(max_range), then
    select_matching (bow=None) or select_matching_and_bow (bow = [(bow_score, candidate index), ...] in query order; only the candidates
    it names are aligned).  `target` and every candidate is a host cloud or the id of a resident keyframe.  The engine's parameters are the registration's (resolution, epsilon, iterations, search method).
    Returns select_*'s tuple: (candidate index or None, relative pose, best score, aligns the sequential reference would have run)."""
    K = len(candidates)
    if K == 0:
        return None, None, DBL_MAX, 0                   # (the reference returns nullptr for no candidates)
    G = np.asarray(guesses, np.float32)
    if G.shape != (K, 4, 4):
        raise ValueError(f"guesses must be [{K},4,4]")
    slots = list(range(K)) if bow is None else list(dict.fromkeys(int(c) for _, c in bow))
    if not slots:
        return None, None, DBL_MAX, 0
    # a keyframe is a host cloud ([N,>=3] array) or the id (int) of a keyframe resident in the engine's store (Engine.window_keyframe /
    # keyframe_add): ids go into the batch rows device to device, arrays are uploaded as before
    is_id = lambda c: isinstance(c, (int, np.integer))
    size = lambda c: engine.keyframe_get(c, fetch=False) if is_id(c) else len(c)
    tgt = target if is_id(target) else ndt._as_points(target)
    srcs = [candidates[c] if is_id(candidates[c]) else ndt._as_points(candidates[c]) for c in slots]
    engine.batch_reserve(len(slots), max(size(tgt), 1), max(max(size(s) for s in srcs), 1))
    for k, s in enumerate(srcs):
        (engine.batch_set_target_keyframe if is_id(tgt) else engine.batch_set_target)(k, tgt)
        (engine.batch_set_source_keyframe if is_id(s) else engine.batch_set_source)(k, s)
    res = engine.batch_align(G[slots])
    sc, _ = engine.batch_fitness_scores(max_range)
    converged, scores, finals = [False] * K, [DBL_MAX] * K, [None] * K
    for k, c in enumerate(slots):
        converged[c], scores[c], finals[c] = res[k]["converged"], float(sc[k]), res[k]["final"]
    if bow is None:
        return select_matching(converged, scores, finals, thresh)
    return select_matching_and_bow(converged, scores, finals, bow, thresh)


LATTICE_DX = LATTICE_DY = (-2.0, -1.0, 0.0, 1.0, 2.0)      # [m]  pose_lattice's default offsets: two leaves of a 1 m grid either way ...
LATTICE_DYAW = (-0.1, 0.0, 0.1)                            # [rad] ... and a yaw step that moves a point 30 m out by three of them


def pose_lattice(guess, dx=LATTICE_DX, dy=LATTICE_DY, dyaw=LATTICE_DYAW) -> np.ndarray:
    """Start poses around a loop guess: [G,4,4] float32.  Entry 0 is the guess itself, bit for bit; then, for every (ddx, ddy, psi) of
    dx x dy x dyaw in that order except (0, 0, 0), [Rz(psi) R | t + (ddx, ddy, 0)] from the guess's R and t -- computed in f64, cast once,
    last row exactly 0 0 0 1.  Not in the reference, whose loop check has the one guess (loop_detector.hpp:171-172)."""
    g32 = np.array(guess, np.float32)
    if g32.shape != (4, 4):
        raise ValueError("guess must be 4x4")
    G64 = g32.astype(np.float64)
    off = np.array([(x, y, p) for x in dx for y in dy for p in dyaw if not (x == 0 and y == 0 and p == 0)], np.float64).reshape(-1, 3)
    c, s = np.cos(off[:, 2:3]), np.sin(off[:, 2:3])
    # Rz(psi) R row by row -- rows 0 and 1 of R mixed, row 2 kept -- each entry two products and one sum, rounded where they stand
    P = np.zeros((len(off), 4, 4))
    P[:, 0, :3] = c * G64[0, :3] - s * G64[1, :3]
    P[:, 1, :3] = s * G64[0, :3] + c * G64[1, :3]
    P[:, 2, :3] = G64[2, :3]
    P[:, :3, 3] = G64[:3, 3]
    P[:, :2, 3] += off[:, :2]
    P32 = P.astype(np.float32)
    P32[:, 3] = np.float32([0, 0, 0, 1])
    return np.concatenate([g32[None], P32])


def pick_starts(scores) -> list[int]:
    """Per row of scores [K,G] (candidate k, lattice pose j) the lattice index of the highest score; a tie goes to the lowest index, so the
    guess (index 0) wins ties and wins when nothing hits."""
    S = np.asarray(scores, np.float64)
    return [int(np.argmax(row)) for row in S.reshape(S.shape[0], -1)]


def verify_candidates_search(engine: ndt.Engine, target, candidates, guesses, lattice=None, max_range: float = float("inf"), thresh: float = 0.5,
                             bow=None):
    """verify_candidates with a search over start poses in front of the aligns: the slots are filled as verify_candidates fills them, ONE
    batch_score_poses scores pose_lattice(guesses[c], **lattice) for every candidate c (lattice: a dict of pose_lattice's dx / dy / dyaw,
    None = its defaults), every candidate starts from its best-scoring pose (pick_starts), and from there on it is verify_candidates' own
    flow: ONE batch_align, ONE batch_fitness_scores, select_matching or select_matching_and_bow.  NDT at 0.5-1 m leaves converges from a
    metre or two; a loop guess after a long loop is often further off, and the reference's fitness threshold then turns the missed basin
    into a missed loop.  This is NOT in the reference; a lattice of one pose (dx = dy = dyaw = (0,)) is verify_candidates word for word.
    Returns verify_candidates' tuple plus the picked lattice index of every candidate (None for one that `bow` does not name)."""
    K = len(candidates)
    if K == 0:
        return None, None, DBL_MAX, 0, []
    G = np.asarray(guesses, np.float32)
    if G.shape != (K, 4, 4):
        raise ValueError(f"guesses must be [{K},4,4]")
    slots = list(range(K)) if bow is None else list(dict.fromkeys(int(c) for _, c in bow))
    if not slots:
        return None, None, DBL_MAX, 0, [None] * K
    is_id = lambda c: isinstance(c, (int, np.integer))
    size = lambda c: engine.keyframe_get(c, fetch=False) if is_id(c) else len(c)
    tgt = target if is_id(target) else ndt._as_points(target)
    srcs = [candidates[c] if is_id(candidates[c]) else ndt._as_points(candidates[c]) for c in slots]
    engine.batch_reserve(len(slots), max(size(tgt), 1), max(max(size(s) for s in srcs), 1))
    for k, s in enumerate(srcs):
        (engine.batch_set_target_keyframe if is_id(tgt) else engine.batch_set_target)(k, tgt)
        (engine.batch_set_source_keyframe if is_id(s) else engine.batch_set_source)(k, s)
    L = np.stack([pose_lattice(G[c], **(lattice or {})) for c in slots])               # [slots, n_poses, 4, 4]
    n_poses = L.shape[1]
    sc_l, _ = engine.batch_score_poses(np.repeat(np.arange(len(slots)), n_poses), L.reshape(-1, 4, 4))
    picked = pick_starts(sc_l.reshape(len(slots), n_poses))
    res = engine.batch_align(L[np.arange(len(slots)), picked])
    sc, _ = engine.batch_fitness_scores(max_range)
    converged, scores, finals, picks = [False] * K, [DBL_MAX] * K, [None] * K, [None] * K
    for k, c in enumerate(slots):
        converged[c], scores[c], finals[c], picks[c] = res[k]["converged"], float(sc[k]), res[k]["final"], picked[k]
    if bow is None:
        return (*select_matching(converged, scores, finals, thresh), picks)
    return (*select_matching_and_bow(converged, scores, finals, bow, thresh), picks)


def verify_candidates_ndt(engine: ndt.Engine, target, candidates, guesses, max_range: float = float("inf"), thresh: float = 0.5, bow=None):
    """verify_candidates for registration_method = NDT (pcl::NormalDistributionsTransform, the factory's fall-back): the same arguments, the
    same tuple, on an engine whose MI355NDT_OPT_NDT_CLASS is 1 (registrations.select_registration_method makes one).  The batch surface serves
    the class as it serves ndt_omp, so this is verify_candidates itself; the check only keeps a class-0 engine from answering for NDT."""
    if engine.get_option(ndt.OPT_NDT_CLASS) != ndt.NDT_CLASSES["pcl"]:
        raise ValueError("verify_candidates_ndt needs an engine with OPT_NDT_CLASS = 1")
    return verify_candidates(engine, target, candidates, guesses, max_range, thresh, bow)


def verify_candidates_gicp(engine: ndt.Engine, target, candidates, guesses, max_range: float = float("inf"), thresh: float = 0.5, bow=None):
    """verify_candidates for registration_method = GICP_OMP: the same arguments, the same tuple.  The target becomes the GICP surface's
    target, candidate k the source of slot k of ONE gicp_batch_align (the K optimisers advance in lockstep: mi355ndt_gicp_batch_align),
    then ONE keyframe_fitness_scores([target] * K, candidates, finals, max_range) -- getFitnessScore at each final transformation, the
    kd-tree over the target -- and select_matching / select_matching_and_bow as they are.  Host clouds become keyframes for the call
    (keyframe_add) and are released afterwards.  The engine's GICP parameters (gicp_set_params) are the registration's."""
    return _verify_on_slots(engine, engine.gicp_set_target, engine.gicp_batch_reserve, engine.gicp_batch_set_source, engine.gicp_batch_align,
                            target, candidates, guesses, max_range, thresh, bow)


def verify_candidates_icp(engine: ndt.Engine, target, candidates, guesses, max_range: float = float("inf"), thresh: float = 0.5, bow=None):
    """verify_candidates for registration_method = ICP: the same arguments, the same tuple.  The target becomes the ICP surface's target,
    candidate k the source of slot k of ONE icp_batch_align (mi355ndt_icp_batch_align: one round trip per iteration for all candidates
    that have not ended), then ONE keyframe_fitness_scores and the two selection rules as they are.  The engine's ICP parameters
    (icp_set_params) are the registration's."""
    return _verify_on_slots(engine, engine.icp_set_target, engine.icp_batch_reserve, engine.icp_batch_set_source, engine.icp_batch_align,
                            target, candidates, guesses, max_range, thresh, bow)


def _verify_on_slots(engine, set_target, batch_reserve, batch_set_source, batch_align, target, candidates, guesses, max_range, thresh, bow):
    """the body verify_candidates_gicp and verify_candidates_icp share: the surface's four calls differ, nothing else"""
    K = len(candidates)
    if K == 0:
        return None, None, DBL_MAX, 0
    G = np.asarray(guesses, np.float32)
    if G.shape != (K, 4, 4):
        raise ValueError(f"guesses must be [{K},4,4]")
    slots = list(range(K)) if bow is None else list(dict.fromkeys(int(c) for _, c in bow))
    if not slots:
        return None, None, DBL_MAX, 0
    is_id = lambda c: isinstance(c, (int, np.integer))
    own = []

    def resident(c):
        if is_id(c):
            return int(c)
        own.append(engine.keyframe_add(ndt._as_points(c)))
        return own[-1]
    try:
        tgt = resident(target)
        ids = [resident(candidates[c]) for c in slots]
        set_target(keyframe=tgt)
        batch_reserve(len(slots))
        for k, i in enumerate(ids):
            batch_set_source(k, keyframe=i)
        res = batch_align(G[slots])
        sc, _ = engine.keyframe_fitness_scores([tgt] * len(slots), ids, [r["final"] for r in res], max_range)
    finally:
        for i in own:
            engine.keyframe_release(i)
    converged, scores, finals = [False] * K, [DBL_MAX] * K, [None] * K
    for k, c in enumerate(slots):
        converged[c], scores[c], finals[c] = res[k]["converged"], float(sc[k]), res[k]["final"]
    if bow is None:
        return select_matching(converged, scores, finals, thresh)
    return select_matching_and_bow(converged, scores, finals, bow, thresh)
