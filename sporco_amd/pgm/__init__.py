"""Solver classes mirroring the reference sub-package of the same name."""

from . import bpdn  # noqa: F401
from . import cmod  # noqa: F401
