"""Host-side mirror of pclomp::GeneralizedIterativeClosestPoint (include/ndt_omp/gicp_omp.h) over the C-ABI's GICP surface
(mi355ndt_gicp_*, include/mi355_ndt.h): the registration select_registration_method hands out for registration_method = GICP_OMP
(src/global_graph/registrations.cpp:43-53), with the reference's method names.  The covariances, the correspondences and the cost sums run
in libmi355ndt.so on the GPU; the BFGS optimiser and the outer loop run on the library's host side.  There is no CPU fallback."""
from __future__ import annotations

import numpy as np

from . import ndt


class GeneralizedIterativeClosestPoint:
    """`reg.setInputTarget(..); reg.setInputSource(..); reg.align(guess)` as the loop detector drives it (loop_detector.hpp:219).
    A cloud may also be a resident keyframe: setInputTarget(keyframe=id) -- its covariances then stay with the keyframe."""

    def __init__(self, device: int = 0, engine: ndt.Engine | None = None):
        self._e = engine if engine is not None else ndt.Engine(device=device)
        self._p = ndt.default_gicp_params()
        self._res = None

    @classmethod
    def from_factory(cls, transformation_epsilon: float = 0.01, maximum_iterations: int = 64, gicp_correspondence_randomness: int = 20,
                     gicp_max_optimizer_iterations: int = 20, **kw):
        """the object select_registration_method builds for GICP_OMP (registrations.cpp:46-52), its parameter defaults included"""
        reg = cls(**kw)
        reg.setTransformationEpsilon(transformation_epsilon)
        reg.setMaximumIterations(maximum_iterations)
        reg.setCorrespondenceRandomness(gicp_correspondence_randomness)
        reg.setMaximumOptimizerIterations(gicp_max_optimizer_iterations)
        return reg

    def _push(self):
        self._e.gicp_set_params(self._p)

    def setCorrespondenceRandomness(self, k: int):          # gicp_omp.h: k_correspondences_
        self._p.k_correspondences = int(k)
        self._push()

    def setMaximumOptimizerIterations(self, n: int):        # max_inner_iterations_
        self._p.max_inner_iterations = int(n)
        self._push()

    def setRotationEpsilon(self, eps: float):
        self._p.rotation_epsilon = float(eps)
        self._push()

    def setTransformationEpsilon(self, eps: float):         # pcl::Registration
        self._p.transformation_epsilon = float(eps)
        self._push()

    def setMaximumIterations(self, n: int):                 # pcl::Registration
        self._p.max_iterations = int(n)
        self._push()

    def setMaxCorrespondenceDistance(self, d: float):       # pcl::Registration: corr_dist_threshold_
        self._p.corr_dist_threshold = float(d)
        self._push()

    def setInputTarget(self, cloud=None, keyframe: int | None = None):
        self._e.gicp_set_target(cloud, keyframe)

    def setInputSource(self, cloud=None, keyframe: int | None = None):
        self._e.gicp_set_source(cloud, keyframe)

    def align(self, guess=None) -> np.ndarray:
        """align(output, guess): returns the source moved by the final transformation, [N,3] f32"""
        self._res = self._e.gicp_align(np.eye(4, dtype=np.float32) if guess is None else guess)
        return self._e.gicp_get_aligned()

    def getFinalTransformation(self) -> np.ndarray:
        return self._res["final"] if self._res else np.eye(4, dtype=np.float32)

    def hasConverged(self) -> bool:
        return bool(self._res and self._res["converged"])

    @property
    def result(self) -> dict | None:
        """the last align's record: final, converged, iterations, inner_status, n_matched, delta"""
        return self._res

    @property
    def engine(self) -> ndt.Engine:
        return self._e
