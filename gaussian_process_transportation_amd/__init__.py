"""MI355X-native Gaussian-process transportation hot path (drop-in for the reference's
`policy_transportation` exports: AffineTransform, GaussianProcess, GaussianProcessTransportation)."""
from .affine_transform import AffineTransform
from .gaussian_process import GaussianProcess
from .policy_transportation import PolicyTransportation
from .gaussian_process_transportation import GaussianProcessTransportation
from .svgp_exact import StocasticVariationalGaussianProcess, SVGPExactPredictor
from .svgp_transport import SVGPTransport
from .svgp_surface import StocasticVariationalGaussianProcess as SurfaceSVGP
from .gaussian_process_al import ActiveLearningGaussianProcess
from .gaussian_process_batch import GaussianProcessBatch
from .batch_transportation import GaussianProcessTransportationBatch
from .transport_chain import TransportChain
from .gaussian_process_transportation_diffeomorphic import GaussianProcessTransportationDiffeo
from .posterior_functions import PosteriorFunctions

# the reference's three exports first; then the duck-typed caller, the SVGP exact-conversion path and the
# point-cloud surface SVGP, the large-input exact regressor (greedy active-learning subset selection), and the batch of small
# models (one workgroup each) with its transport protocol, the chain of transports with its one-call pull-back, and the
# reference's fold-free transport (the length-scale ceiling searched and scored on the device), and the whole functions drawn from
# a posterior (GaussianProcess.sample_functions)
__all__ = ["AffineTransform", "GaussianProcessTransportation", "GaussianProcess", "PolicyTransportation",
           "SVGPTransport", "StocasticVariationalGaussianProcess", "SVGPExactPredictor", "SurfaceSVGP",
           "ActiveLearningGaussianProcess", "GaussianProcessBatch", "GaussianProcessTransportationBatch", "TransportChain",
           "GaussianProcessTransportationDiffeo", "PosteriorFunctions"]
