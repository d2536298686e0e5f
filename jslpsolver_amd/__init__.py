"""jslpsolver_amd -- MI355X-native dense-tableau simplex engine behind jsLPSolver's `Solve(model)` API.

Only the hot path lives here: csrc/ (HIP kernels for gfx950 + the C ABI of
include/jslp_engine.h) and the thin host mirror of the reference interface for that path.
"""
from .engine import Tableau, TableauPack, pivot_digest  # noqa: F401
from .model import Model, UnsupportedModel  # noqa: F401
from .solver import Solve, solve_many, solve_packed  # noqa: F401

__all__ = ["Tableau", "TableauPack", "Model", "Solve", "solve_many", "solve_packed", "UnsupportedModel", "pivot_digest"]
