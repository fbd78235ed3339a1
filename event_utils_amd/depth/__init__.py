from . import emvs  # noqa: F401
from . import stereo  # noqa: F401
from . import sgm  # noqa: F401
from . import tracking  # noqa: F401
from . import fusion  # noqa: F401
from .emvs import DSI, DepthMap, depth_planes, packet_transforms, packet_times, dsi_votes, dsi_depth_map, emvs_depth_map, \
    depth_to_points  # noqa: F401
from .stereo import Disparity, quantised_time_surfaces, stereo_cost_volume, stereo_match, stereo_disparity, disparity_to_depth, \
    disparity_depth_map  # noqa: F401
from .sgm import sgm_aggregate, match_cost_volume, sgm_match, sgm_disparity  # noqa: F401
from .tracking import Registration, tracking_surface, reference_points, registration_terms, registration_residuals, register_points, \
    track_poses  # noqa: F401
from .fusion import InverseDepthMap, disparity_inverse_depth, depth_inverse_depth, inverse_depth_depth_map, relative_transforms, \
    propagate_inverse_depth, fuse_inverse_depth, regularise_inverse_depth, fuse_stereo_depth  # noqa: F401
