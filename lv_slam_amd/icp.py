"""Host-side mirror of pcl::IterativeClosestPoint over the C-ABI's ICP surface (mi355ndt_icp_*, include/mi355_ndt.h): the registration
select_registration_method hands out for registration_method = ICP (src/global_graph/registrations.cpp:21-29), with PCL's method names.
The move of the working cloud, the nearest-point search and the sums run in libmi355ndt.so on the GPU; the 3x3 SVD, the convergence criteria
and the loop run on the library's host side.  There is no CPU fallback."""
from __future__ import annotations

import numpy as np

from . import ndt


class IterativeClosestPoint:
    """`reg.setInputTarget(..); reg.setInputSource(..); reg.align(guess)` as the loop detector drives it (loop_detector.hpp:219).
    A cloud may also be a resident keyframe: setInputTarget(keyframe=id)."""

    def __init__(self, device: int = 0, engine: ndt.Engine | None = None):
        self._e = engine if engine is not None else ndt.Engine(device=device)
        self._p = ndt.default_icp_params()
        self._res = None
        self._clouds = [None, None]                 # (target, source) as given: getFitnessScore takes them to the keyframe store
        self._push()

    @classmethod
    def from_factory(cls, transformation_epsilon: float = 0.01, maximum_iterations: int = 64, use_reciprocal_correspondences: bool = False, **kw):
        """the object select_registration_method builds for ICP (registrations.cpp:21-29), its parameter defaults included"""
        reg = cls(**kw)
        reg.setTransformationEpsilon(transformation_epsilon)
        reg.setMaximumIterations(maximum_iterations)
        reg.setUseReciprocalCorrespondences(use_reciprocal_correspondences)
        return reg

    def _push(self):
        self._e.icp_set_params(self._p)

    def _set(self, name, value):
        old = getattr(self._p, name)
        setattr(self._p, name, value)
        try:
            self._push()
        except ndt.NDTError:
            setattr(self._p, name, old)             # (a refused value changes nothing)
            raise

    def setTransformationEpsilon(self, eps: float):
        self._set("transformation_epsilon", float(eps))

    def setMaximumIterations(self, n: int):
        self._set("max_iterations", int(n))

    def setEuclideanFitnessEpsilon(self, eps: float):
        self._set("euclidean_fitness_epsilon", float(eps))

    def setMaxCorrespondenceDistance(self, d: float):       # corr_dist_threshold_
        self._set("corr_dist_threshold", float(d))

    def setUseReciprocalCorrespondences(self, on: bool):    # true is refused: not served
        self._set("use_reciprocal_correspondences", int(bool(on)))

    def setInputTarget(self, cloud=None, keyframe: int | None = None):
        self._e.icp_set_target(cloud, keyframe)
        self._clouds[0] = ("id", int(keyframe)) if keyframe is not None else ("cloud", ndt._as_points(cloud))

    def setInputSource(self, cloud=None, keyframe: int | None = None):
        self._e.icp_set_source(cloud, keyframe)
        self._clouds[1] = ("id", int(keyframe)) if keyframe is not None else ("cloud", ndt._as_points(cloud))

    def align(self, guess=None) -> np.ndarray:
        """align(output, guess): returns the working cloud after the last move (PCL's `output`), [N,3] f32"""
        self._push()
        self._res = self._e.icp_align(np.eye(4, dtype=np.float32) if guess is None else guess)
        return self._e.icp_get_aligned()

    def getFinalTransformation(self) -> np.ndarray:
        return self._res["final"] if self._res else np.eye(4, dtype=np.float32)

    def hasConverged(self) -> bool:
        return bool(self._res and self._res["converged"])

    def getFitnessScore(self, max_range: float = float("inf")) -> float:
        """pcl::Registration::getFitnessScore(max_range) at the final transformation, through keyframe_fitness_scores: the target is
        searched, the source is moved.  Host clouds become keyframes for the call and are released afterwards."""
        if self._clouds[0] is None or self._clouds[1] is None:
            raise ndt.NDTError(-7, "getFitnessScore", "a cloud is not set")
        own, ids = [], []
        try:
            for kind, c in self._clouds:
                if kind == "id":
                    ids.append(c)
                else:
                    own.append(self._e.keyframe_add(c))
                    ids.append(own[-1])
            sc, _ = self._e.keyframe_fitness_scores([ids[0]], [ids[1]], [self.getFinalTransformation().astype(np.float64)], max_range)
        finally:
            for i in own:
                self._e.keyframe_release(i)
        return float(sc[0])

    @property
    def result(self) -> dict | None:
        """the last align's record: final, converged, iterations, state, matches, mse"""
        return self._res

    @property
    def engine(self) -> ndt.Engine:
        return self._e
