"""select_registration_method (src/global_graph/registrations.cpp:15-103), branch for branch: the one place where an lv_slam host chooses the
loop-closure registration, with the same parameter names and the same defaults.

    registration_method        what the reference hands out                                here
    "ICP"                      pcl::IterativeClosestPoint                                  icp.IterativeClosestPoint
    holds "GICP", no "OMP"     pcl::GeneralizedIterativeClosestPoint (single-threaded)     NotImplementedError: not served
    holds "GICP" and "OMP"     pclomp::GeneralizedIterativeClosestPoint                    gicp.GeneralizedIterativeClosestPoint
    anything else, no "OMP"    pcl::NormalDistributionsTransform (with a warning when      ndt.NormalDistributionsTransform(ndt_class="pcl")
                               the name does not hold "NDT": a misspelt name ends here)
    anything else with "OMP"   pclomp::NormalDistributionsTransform                        ndt.NormalDistributionsTransform()

`plan_registration` is the decision alone (a pure function of the parameters: what a test without a GPU can walk through);
`select_registration_method` builds the object the plan names.  The matches are the reference's: `==` for ICP, substring search, case-sensitive,
for the others -- "ndt" holds no "NDT", is warned about and gets PCL's NDT like any unknown name.
"""
from __future__ import annotations

import sys
from dataclasses import dataclass, field

from . import gicp, icp, ndt

DEFAULT_METHOD = "NDT_OMP"                      # registrations.cpp:20
SEARCH_METHODS = {"KDTREE": ndt.KDTREE, "DIRECT1": ndt.DIRECT1}      # registrations.cpp:85-96: anything else is DIRECT7


@dataclass
class RegistrationPlan:
    kind: str                                   # "ICP" | "GICP" | "GICP_OMP" | "NDT" | "NDT_OMP"
    settings: dict = field(default_factory=dict)  # every value the branch reads from the parameters, defaults applied
    warnings: list = field(default_factory=list)  # the lines the reference writes to std::cerr
    banner: str = ""                            # the line it writes to std::cout


def plan_registration(params: dict) -> RegistrationPlan:
    """which branch of registrations.cpp:15-103 the parameters take, and what that branch reads"""
    get = params.get
    method = str(get("registration_method", DEFAULT_METHOD))
    common = dict(transformation_epsilon=float(get("transformation_epsilon", 0.01)), maximum_iterations=int(get("maximum_iterations", 64)))
    if method == "ICP":                                                                     # :21-29
        return RegistrationPlan("ICP", dict(common, use_reciprocal_correspondences=bool(get("use_reciprocal_correspondences", False))), [], "registration: ICP")
    if "GICP" in method:                                                                    # :30-54
        s = dict(common, use_reciprocal_correspondences=bool(get("use_reciprocal_correspondences", False)),
                 gicp_correspondence_randomness=int(get("gicp_correspondence_randomness", 20)),
                 gicp_max_optimizer_iterations=int(get("gicp_max_optimizer_iterations", 20)))
        kind = "GICP_OMP" if "OMP" in method else "GICP"
        return RegistrationPlan(kind, s, [], "registration: " + kind)
    warnings = []
    if "NDT" not in method:                                                                 # :57-61
        warnings = [f"warning: unknown registration type({method})", "       : use NDT"]
    res = float(get("ndt_resolution", 0.5))                                                 # :63
    if "OMP" not in method:                                                                 # :64-72
        return RegistrationPlan("NDT", dict(common, ndt_resolution=res), warnings, f"registration: NDT {res:g}")
    threads = int(get("ndt_num_threads", 0))                                                # :75-76
    search = str(get("ndt_nn_search_method", "DIRECT7"))
    s = dict(common, ndt_resolution=res, ndt_num_threads=threads, ndt_nn_search_method=search, neighbor_mode=SEARCH_METHODS.get(search, ndt.DIRECT7))
    return RegistrationPlan("NDT_OMP", s, warnings, f"registration: NDT_OMP {search} {res:g} ({threads} threads)")


def select_registration_method(params: dict, engine=None):
    """The registration object for `params` (a dict with the reference's parameter names; a missing name takes the reference's default).
    `engine`: an ndt.Engine to build the object on (its keyframe store is then shared with the caller), else the object makes its own.
    The warning lines go to stderr and the banner to stdout, as in the reference."""
    plan = plan_registration(params)
    for line in plan.warnings:
        print(line, file=sys.stderr)
    print(plan.banner)
    s = plan.settings
    kw = {} if engine is None else {"engine": engine}
    if plan.kind == "ICP":
        return icp.IterativeClosestPoint.from_factory(s["transformation_epsilon"], s["maximum_iterations"], s["use_reciprocal_correspondences"], **kw)
    if plan.kind == "GICP":
        raise NotImplementedError("registration_method = GICP (pcl::GeneralizedIterativeClosestPoint, PCL's single-threaded class) is not served; "
                                  "GICP_OMP is")
    if plan.kind == "GICP_OMP":
        if s["use_reciprocal_correspondences"]:
            raise NotImplementedError("GICP_OMP with use_reciprocal_correspondences = true is not served")
        return gicp.GeneralizedIterativeClosestPoint.from_factory(s["transformation_epsilon"], s["maximum_iterations"], s["gicp_correspondence_randomness"],
                                                                  s["gicp_max_optimizer_iterations"], **kw)
    if plan.kind == "NDT":                                                                  # pcl::NormalDistributionsTransform, registrations.cpp:66-71
        reg = ndt.NormalDistributionsTransform(ndt_class="pcl", **kw)
    else:                                                                                   # pclomp::NormalDistributionsTransform, registrations.cpp:78-98
        reg = ndt.NormalDistributionsTransform(**kw)
        if s["ndt_num_threads"] > 0:
            reg.setNumThreads(s["ndt_num_threads"])
    reg.setTransformationEpsilon(s["transformation_epsilon"])
    reg.setMaximumIterations(s["maximum_iterations"])
    reg.setResolution(s["ndt_resolution"])
    if plan.kind == "NDT_OMP":
        reg.setNeighborhoodSearchMethod(s["neighbor_mode"])
    return reg
