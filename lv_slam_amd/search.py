"""Host-side mirror of pcl::KdTreeFLANN over the C-ABI's search surface (mi355ndt_keyframe_knn / _radius_search, include/mi355_ndt.h), with
PCL's method names.  The searched cloud is a resident keyframe: a host cloud given to setInputCloud becomes one this object owns and releases,
`keyframe=` names one it does not.  The search runs in libmi355ndt.so on the GPU, exactly (tools/knn_ref.py restates every word); a tie goes
to the lower point id -- FLANN's order among equal distances is not reproduced.  There is no CPU fallback."""
from __future__ import annotations

import numpy as np

from . import ndt


class KdTreeFLANN:
    """`tree.setInputCloud(cloud); ids, d2 = tree.nearestKSearch(queries, k)` for any number of queries at once."""

    def __init__(self, device: int = 0, engine: ndt.Engine | None = None):
        self._e = engine if engine is not None else ndt.Engine(device=device)
        self._own_engine = engine is None
        self._kid = None
        self._owned = False

    def _drop(self):
        if self._kid is not None and self._owned:
            self._e.keyframe_release(self._kid)
        self._kid, self._owned = None, False

    def setInputCloud(self, cloud=None, keyframe: int | None = None):
        """a host cloud ([N,>=3] floats), uploaded once into a keyframe of this object's own; or keyframe=id, borrowed"""
        if (cloud is None) == (keyframe is None):
            raise ValueError("setInputCloud takes a cloud or keyframe=id")
        kid, owned = (int(keyframe), False) if keyframe is not None else (self._e.keyframe_add(cloud), True)
        self._drop()
        self._kid, self._owned = kid, owned

    @property
    def keyframe(self) -> int | None:
        return self._kid

    @property
    def engine(self) -> ndt.Engine:
        return self._e

    def _need(self) -> int:
        if self._kid is None:
            raise ndt.NDTError(-7, "KdTreeFLANN", "no input cloud is set")
        return self._kid

    def nearestKSearch(self, queries, k: int, T=None):
        """(k_indices [n,k] int32, k_sqr_distances [n,k] float32); a query that finds fewer than k points leaves -1 / +inf behind them"""
        ids, d2, _ = self._e.keyframe_knn(self._need(), np.atleast_2d(np.asarray(queries, np.float32)), k, T=T)
        return ids, d2

    def radiusSearch(self, queries, radius: float, max_nn: int, T=None):
        """(k_indices [n,max_nn], k_sqr_distances [n,max_nn], found [n]): found = every point with d2 < radius^2 (strict), the lists hold
        the max_nn nearest of them"""
        return self._e.keyframe_radius_search(self._need(), np.atleast_2d(np.asarray(queries, np.float32)), radius, max_nn, T=T)

    def close(self):
        self._drop()
        if self._own_engine and self._e is not None:
            self._e.close()
        self._e = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            if self._e is not None:
                self._drop()
        except Exception:
            pass
