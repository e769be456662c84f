"""Information matrices of the global graph's edges, ROS-free: include/global_graph/information_matrix_calculator.hpp and
src/global_graph/information_matrix_calculator.cpp over resident keyframes.

The reference calls `calc_information_matrix(cloud1, cloud2, relpose)` once per edge: for the odometry edge of every new keyframe
(GlobalGraphNodelet::flush_keyframe_queue, global_graph_nodelet.cpp:298) and for every accepted loop (optimization_timer_callback, :697).
Each call builds a kd-tree over one window map and queries it with the other.  Here the callers hand over ALL the edges of a flush (or of
a loop block) as (id1, id2, relpose) triples; the fitness scores come from ONE engine call over the keyframes' ids
(Engine.keyframe_fitness_scores: nothing is downloaded or uploaded) and the weighting is the reference's host arithmetic
(ndt.information_matrix).
"""
from __future__ import annotations

import numpy as np

from . import ndt


class InformationMatrixCalculator:
    """Holds the reference's parameters, with its constructor's defaults (information_matrix_calculator.cpp:11-20); keyword arguments
    override them.  `max_range` is calc_fitness_score's (its default: std::numeric_limits<double>::max())."""

    def __init__(self, max_range: float = float("inf"), **params):
        self.params = ndt.default_inf_params(**params)
        self.max_range = float(max_range)

    @property
    def use_const_inf_matrix(self) -> bool:
        return bool(self.params.use_const_inf_matrix)

    def calc_information_matrices(self, engine, edges) -> list:
        """edges: (id1, id2, relpose) triples -- keyframe id1 is the searched cloud, keyframe id2 is moved by relpose (4x4 f64).  One engine
        call for all of them; returns one 6x6 f64 matrix per edge.  With use_const_inf_matrix the engine is not called at all."""
        edges = list(edges)
        if not edges:
            return []
        if self.use_const_inf_matrix:
            m = ndt.information_matrix(0.0, self.params)
            return [m.copy() for _ in edges]
        ids1 = [int(e[0]) for e in edges]
        ids2 = [int(e[1]) for e in edges]
        rel = np.stack([np.asarray(e[2], np.float64).reshape(4, 4) for e in edges])
        scores, _ = engine.keyframe_fitness_scores(ids1, ids2, rel, self.max_range)
        return [ndt.information_matrix(float(s), self.params) for s in scores]

    def calc_information_matrix(self, engine, id1: int, id2: int, relpose) -> np.ndarray:
        """The one-edge form: calc_information_matrix(cloud1, cloud2, relpose) of the reference over ids."""
        return self.calc_information_matrices(engine, [(id1, id2, relpose)])[0]
