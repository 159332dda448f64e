"""Analysis classes of the hot path (mirrors ``mdhelper.analysis``)."""

from . import (angle, base, cluster, dihedral, dynamics, electrostatics, hbond, order, polymer, profile,  # noqa: F401
               spatial, structure, transport)
from .structure import (IntermediateScatteringFunction, RadialDistributionFunction,  # noqa: F401
                        StructureFactor)
from .angle import AngularDistribution  # noqa: F401
from .cluster import Clusters  # noqa: F401
from .dihedral import Dihedrals  # noqa: F401
from .dynamics import (DistinctVanHove, FourPointSusceptibility, OrientationalRelaxation,  # noqa: F401
                       PairResidence, VanHove, calculate_four_point_susceptibility,
                       calculate_non_gaussian_parameter, calculate_residence_time)
from .electrostatics import DipoleMoment, calculate_relative_permittivity  # noqa: F401
from .hbond import HydrogenBonds  # noqa: F401
from .order import BondOrientationalOrder, TetrahedralOrder  # noqa: F401
from .polymer import (EndToEndVector, Gyradius, InternalDistances, RouseModes,  # noqa: F401
                      SingleChainStructureFactor)
from .profile import DensityProfile, calculate_potential_profile  # noqa: F401
from .spatial import SpatialDistributionFunction  # noqa: F401
from .transport import Onsager  # noqa: F401
