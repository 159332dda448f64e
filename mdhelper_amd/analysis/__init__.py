"""Analysis classes of the hot path (mirrors ``mdhelper.analysis``)."""

from . import base, polymer, profile, structure, transport  # noqa: F401
from .structure import (IntermediateScatteringFunction, RadialDistributionFunction,  # noqa: F401
                        StructureFactor)
from .polymer import EndToEndVector, Gyradius, SingleChainStructureFactor  # noqa: F401
from .profile import DensityProfile, calculate_potential_profile  # noqa: F401
from .transport import Onsager  # noqa: F401
